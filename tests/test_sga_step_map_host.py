"""Host half of SGA iterative inference on a step map: the weight of every latent position, the weighted
distortion D_w and J of ``coded_cost(weighted=True)``, and the refusals of ``compress(x, itinf=dict(step_offsets=...))`` /
``initialize_itinf(step_offsets=...)`` -- every one of them before anything is launched.  No GPU: the model is the stand-in of
test_sga_step_host.py, whose first device call raises."""
import re
from pathlib import Path

import numpy as np
import pytest

from test_sga_step_host import Launched, X, stand_in

ROOT = Path(__file__).resolve().parent.parent
MAP_ENTRY_POINTS = ("sntc_sga_normal_step_map_fwd", "sntc_sga_normal_step_map_bwd")
ENTRY_POINTS = MAP_ENTRY_POINTS + ("sntc_distortion_grad_weighted", "sntc_block_sse")


def test_entry_points_declared_bound_and_exported():
    from shallow_ntc_amd import _capi
    header = (ROOT / "include" / "sntc.h").read_text()
    lib = _capi.load()
    for name in ENTRY_POINTS:
        at = re.search(rf"/\*(?:(?!\*/).)*\*/\s*int {name}\(", header, re.S)
        assert at, f"{name} is not declared in include/sntc.h"
        if name in MAP_ENTRY_POINTS:                                # the siblings' citations
            assert "mshyper/models.py:285-291" in at.group(0) and "common/latent_rvs_utils.py:8-48" in at.group(0)
        assert name in _capi.SIGNATURES and hasattr(lib, name)
        assert _capi.SIGNATURES[name][1][-1] is _capi.C.c_void_p
    # one copy of the map's clamp and table layout: the header, read by the coder's map kernels and by the SGA ones
    rules = (ROOT / "shallow-ntc_amd" / "csrc" / "step_rules.h").read_text()
    assert "int map_index(" in rules
    for src in ("quant_step.hip", "sga.hip"):
        text = (ROOT / "shallow-ntc_amd" / "csrc" / src).read_text()
        assert '#include "step_rules.h"' in text and "int map_index(" not in text and "map_index(" in text


# ---- position_weights ---------------------------------------------------------------------------------------------------------
def test_position_weights():
    from shallow_ntc_amd import entropy_coding as ec
    from shallow_ntc_amd.mshyper.models import step_lambdas
    for k in (ec.STEP_MIN, -6, 0, 5, ec.STEP_MAX):
        w = ec.position_weights(np.full((2, 3, 5), k, np.int8))
        assert w.shape == (2, 3, 5) and w.dtype == np.float64
        assert (w == step_lambdas(1.0, [k])[0]).all()              # float equality with the per-image rule
    ladder = np.arange(ec.STEP_MIN, ec.STEP_MAX + 1, dtype=np.int8).reshape(1, 1, -1)
    w = ec.position_weights(ladder)[0, 0]
    assert (np.diff(w) < 0).all() and w[-ec.STEP_MIN] == 1.0      # a finer step weighs its pixels more; index 0 weighs 1
    assert 1 / 2700 < w[-1] and w[0] < 2700                        # the range the kernel tests draw their weights from
    mixed = np.array([[[-32, 0], [7, 32]]], np.int8)
    assert ec.position_weights(mixed).tolist() == [[[1 / ec.step_size(-32) ** 2, 1.0], [1 / ec.step_size(7) ** 2, 1 / ec.step_size(32) ** 2]]]
    for bad in (np.zeros((2, 3), np.int8), np.zeros((1, 2, 2), np.int32), np.full((1, 2, 2), 33, np.int8), np.full((1, 1, 1), -33, np.int8)):
        with pytest.raises(ValueError):
            ec.position_weights(bad)


# ---- D_w and J ------------------------------------------------------------------------------------------------------------------
def test_weighted_distortion_arithmetic():
    from shallow_ntc_amd import entropy_coding as ec
    from shallow_ntc_amd.mshyper.models import step_lambdas, weighted_distortion
    # by hand: two images of 2 x 2 blocks
    sse = np.array([[[10, 20], [30, 40]], [[1, 0], [0, 3]]], np.int64)
    w = np.array([[[1.0, 0.5], [2.0, 0.25]], [[4.0, 9.0], [9.0, 1.0]]])
    got = weighted_distortion(sse, w, 100)
    assert got.dtype == np.float64 and got.tolist() == [(10 + 10 + 60 + 10) / 100.0, (4 + 3) / 100.0]
    # weights may cover more positions than there are pixel blocks (positions wholly in the padding): the extra ones are unused
    wide = np.full((2, 3, 4), 1e9)
    wide[:, :2, :2] = w
    assert weighted_distortion(sse, wide, 100).tolist() == got.tolist()
    with pytest.raises(ValueError):
        weighted_distortion(sse, w[:, :1], 100)
    # a constant map: lambda_i D_i of the per-image rule, and J with it
    rng = np.random.default_rng(0)
    H, W, C, lam = 60, 64, 3, 0.02
    blocks = rng.integers(0, 16 * 16 * 3 * 255 ** 2, size=(3, 4, 4))
    bits = rng.uniform(1e3, 1e5, size=3)
    for ks in ([-32, 0, 32], [-6, 5, 17]):
        K = np.array(ks, np.int8).reshape(3, 1, 1) * np.ones((3, 4, 4), np.int8)
        d_w = weighted_distortion(blocks, ec.position_weights(K), H * W * C)
        want = step_lambdas(lam, ks) * (blocks.sum(axis=(1, 2)) / float(H * W * C))
        np.testing.assert_allclose(lam * d_w, want, rtol=1e-15, atol=0.0)
        np.testing.assert_allclose(bits / (H * W) + lam * d_w, bits / (H * W) + want, rtol=1e-15, atol=0.0)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def map_stand_in(**over):
    """The stand-in of test_sga_step_host.py plus the host half of the map."""
    from shallow_ntc_amd.mshyper.models import Model
    stub = stand_in(**over)
    type(stub)._itinf_grid_of = Model._itinf_grid_of
    return stub


OFF = np.zeros((2, 4, 4), np.int8)


def test_map_refusals_come_before_any_launch():
    model = map_stand_in()
    with pytest.raises(Launched):                                  # the stand-in works: a valid call reaches the device
        model.compress(X, itinf=dict(steps=2, step=[3, -3], step_offsets=OFF))
    with pytest.raises(Launched):
        model.compress(X, itinf=dict(steps=2, target_bpp=0.3, step_offsets=OFF))
    with pytest.raises(Launched):
        model.initialize_itinf(X, step=1, step_offsets=OFF)
    for bad in (0.1, [0.1, 0.2], 0.0, float("nan")):              # rd_lambda with a map, valid or not
        with pytest.raises(ValueError, match="rd_lambda"):
            model.compress(X, itinf=dict(steps=2, rd_lambda=bad, step_offsets=OFF))
        with pytest.raises(ValueError, match="rd_lambda"):
            model.compress(X, itinf=dict(steps=2, step=1, rd_lambda=bad, step_offsets=OFF))
        with pytest.raises(ValueError, match="rd_lambda"):
            model.initialize_itinf(X, rd_lambda=bad, step_offsets=OFF)
    with pytest.raises(ValueError, match="exclude"):
        model.compress(X, itinf=dict(steps=2, step=1, target_bpp=0.3, step_offsets=OFF))
    for bad in (33, [1], [1, 2.0]):
        with pytest.raises(ValueError):
            model.compress(X, itinf=dict(steps=2, step=bad, step_offsets=OFF))
        with pytest.raises(ValueError):
            model.initialize_itinf(X, step=bad, step_offsets=OFF)
    ssim = map_stand_in(_distortion="ms_ssim")
    with pytest.raises(NotImplementedError, match="ms_ssim"):
        ssim.compress(X, itinf=dict(steps=2, step_offsets=OFF))
    with pytest.raises(NotImplementedError, match="ms_ssim"):
        ssim.initialize_itinf(X, step_offsets=OFF)
    fact = map_stand_in(factorized=True)
    with pytest.raises(NotImplementedError, match="hyperprior"):
        fact.compress(X, itinf=dict(steps=2, step_offsets=OFF))
    with pytest.raises(NotImplementedError, match="hyperprior"):
        fact.initialize_itinf(X, step_offsets=OFF)
    split = map_stand_in(_precision="bf16x3")
    with pytest.raises(NotImplementedError, match="fp32"):
        split.compress(X, itinf=dict(steps=2, step_offsets=OFF))
    with pytest.raises(NotImplementedError, match="fp32"):
        split.initialize_itinf(X, step_offsets=OFF)
    # the exclusion at the top level stays, and an unknown key is still an error
    with pytest.raises(ValueError, match="itinf"):
        model.compress(X, itinf=dict(steps=2), step_offsets=OFF)
    with pytest.raises(ValueError, match="itinf"):
        model.compress(X, itinf=dict(steps=2, step_offsets=OFF), step_offsets=OFF)
    with pytest.raises(TypeError):
        model.compress(X, itinf=dict(steps=2, step_offset=OFF))


def test_offsets_are_checked_before_any_launch():
    """Wrong shape, dtype and range (``check_offsets``) on a stand-in that knows its latent shapes and nothing else of the device."""
    from shallow_ntc_amd.mshyper.models import Model

    class Shapes:
        def latent_shapes(self, H, W):
            return (8, 8, 1, 1, 4, 4)

    model = map_stand_in(downsample_factor=64)
    type(model)._position_block = Model._position_block
    type(model)._get_codec = lambda self: Shapes()
    with pytest.raises(Launched):                                  # valid offsets pass the host half and reach the device
        model.compress(X, itinf=dict(steps=2, step_offsets=OFF))
    for bad in (np.zeros((2, 4, 5), np.int8), np.zeros((1, 4, 4), np.int8), np.zeros((2, 4, 4), np.float32),
                np.zeros((2, 4, 4), bool), np.full((2, 4, 4), 65), np.full((2, 4, 4), -65)):
        with pytest.raises(ValueError, match="step_offsets"):
            model.compress(X, itinf=dict(steps=2, step_offsets=bad))
        with pytest.raises(ValueError, match="step_offsets"):
            model.initialize_itinf(X, step_offsets=bad)
    # the pixel block of a position: padded size over latent size, refused where that is not a whole square
    assert model._position_block(64, 64) == 16 and model._position_block(60, 64) == 16
    type(model)._get_codec = lambda self: type("S", (), dict(latent_shapes=lambda s, H, W: (8, 8, 1, 1, 3, 4)))()
    with pytest.raises(ValueError, match="block"):
        model.compress(X, itinf=dict(steps=2, step_offsets=np.zeros((2, 3, 4), np.int8)))
