"""Host half of iterative inference at a quantisation step: each image's lambda, the selection rule with and
without a bit budget, and the refusals of ``compress(x, itinf=dict(step / target_bpp / rd_lambda))`` -- every one of them before
anything is launched.  No GPU: the model is a stand-in whose first device call raises."""
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
ENTRY_POINTS = ("sntc_sga_normal_step_fwd", "sntc_sga_normal_step_bwd")


def test_entry_points_declared_bound_and_exported():
    from shallow_ntc_amd import _capi
    header = (ROOT / "include" / "sntc.h").read_text()
    lib = _capi.load()
    for name in ENTRY_POINTS:
        at = re.search(rf"/\*(?:(?!\*/).)*\*/\s*int {name}\(", header, re.S)
        assert at, f"{name} is not declared in include/sntc.h"
        assert "mshyper/models.py:285-291" in at.group(0) and "common/latent_rvs_utils.py:8-48" in at.group(0)
        assert name in _capi.SIGNATURES and hasattr(lib, name)
        assert _capi.SIGNATURES[name][1][-1] is _capi.C.c_void_p
    makefile = (ROOT / "shallow-ntc_amd" / "csrc" / "Makefile").read_text()
    assert "step_rules.h" in makefile
    # one copy of the step rule: the header, included by both users
    for src in ("quant_step.hip", "sga.hip"):
        text = (ROOT / "shallow-ntc_amd" / "csrc" / src).read_text()
        assert '#include "step_rules.h"' in text and "float step_diff(" not in text


def test_default_lambda_and_override():
    from shallow_ntc_amd import entropy_coding as ec
    from shallow_ntc_amd.mshyper.models import step_lambdas
    ks = [-32, -6, 0, 6, 32]
    lams = step_lambdas(0.02, ks)
    assert lams.dtype == np.float64 and lams.tolist() == [0.02 / ec.step_size(k) ** 2 for k in ks]
    assert lams[2] == 0.02 and lams[1] > 0.02 > lams[3]            # a finer step weighs the distortion more
    # lambda_i Delta_i^2 is the same for every step: the slope -dR/dD of the high-resolution regime
    np.testing.assert_allclose(lams * np.array([ec.step_size(k) for k in ks]) ** 2, 0.02, rtol=1e-15)
    assert step_lambdas(0.02, ks, 0.5).tolist() == [0.5] * 5
    assert step_lambdas(0.02, [1, 2], [0.25, 3.0]).tolist() == [0.25, 3.0]
    assert step_lambdas(0.02, [1, 2], np.float32(0.5)).tolist() == [0.5, 0.5]
    for bad in (0.0, -1.0, float("nan"), float("inf"), [0.1], [0.1, 0.2, 0.3], [0.1, 0.0], [0.1, float("inf")], "x", [[0.1, 0.2]]):
        with pytest.raises(ValueError, match="rd_lambda"):
            step_lambdas(0.02, [1, 2], bad)


def test_selection_rule_without_a_budget():
    from shallow_ntc_amd.mshyper.models import candidate_wins
    got = candidate_wins([1.0, 2.0, 3.0], [9, 9, 9], [2.0, 2.0, 2.0], [1, 1, 1])
    assert got.tolist() == [True, False, False]                   # strictly smaller J only: the earlier candidate wins a tie


def test_eligibility_rule():
    """Scripted (J, bits) per image against budgets, 100 flushed bits: where the start candidate fits (met), a candidate must
    fit too and then wins by J; where nothing fits, the fewest bits win whatever J says."""
    from shallow_ntc_amd.mshyper.models import candidate_wins
    flushed = 100.0
    budget = np.array([1000.0, 1000.0, 1000.0, 1000.0, 1000.0, 50.0, 50.0, 50.0])
    met = np.array([True, True, True, True, True, False, False, False])
    j_best = np.array([5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0])
    bits_best = np.array([800.0] * 5 + [400.0] * 3)
    #                 fits+better  fits+worse  over+better  exactly-at  tie-J     fewer bits  more bits(J better)  equal bits
    j_cand = np.array([4.0,        6.0,        1.0,         4.0,        5.0,      9.0,        1.0,                 1.0])
    bits_cand = np.array([850.0,   700.0,      900.5,       900.0,      100.0,    399.0,      401.0,               400.0])
    got = candidate_wins(j_cand, bits_cand, j_best, bits_best, budget, flushed, met)
    assert got.tolist() == [True, False, False, True, False, True, False, False]
    # the over-budget candidate with the smaller J (image 2) is not taken; without the budget it would be
    assert candidate_wins(j_cand, bits_cand, j_best, bits_best)[2]


class Launched(Exception):
    pass


def stand_in(**over):
    """What ``_compress_itinf`` and ``initialize_itinf`` read before they touch the device; the first device call raises."""
    from shallow_ntc_amd.mshyper.models import Model

    class Stub:
        _latent_config = dict(uq=dict(method="sga"))
        _optimizer_config = {}
        _precision = "fp32"
        _distortion = "mse"
        _rd_lambda = 0.02
        factorized = False
        _itinf_grid_of = Model._itinf_grid_of
        compress = Model.compress
        _check_step_arguments = Model._check_step_arguments
        _compress_itinf = Model._compress_itinf
        initialize_itinf = Model.initialize_itinf

        def _as_device_images(self, x):
            raise Launched

        def infer_latent_rvs(self, x):
            raise Launched

        def _get_codec(self):
            raise Launched

    stub = Stub()
    for k, v in over.items():
        setattr(stub, k, v)
    return stub


X = np.zeros((2, 64, 64, 3), np.float32)


def test_refusals_come_before_any_launch():
    model = stand_in()
    with pytest.raises(Launched):                                  # the stand-in works: a valid call reaches the device
        model.compress(X, itinf=dict(steps=2, step=[3, -3]))
    with pytest.raises(Launched):
        model.compress(X, itinf=dict(steps=2, target_bpp=0.3, rd_lambda=[0.1, 0.2]))
    with pytest.raises(ValueError, match="exclude"):
        model.compress(X, itinf=dict(steps=2, step=1, target_bpp=0.3))
    for bad in (33, -33, [1, 33], [1], [1, 2, 3], 1.5, [1, 2.0]):
        with pytest.raises(ValueError):
            model.compress(X, itinf=dict(steps=2, step=bad))
        with pytest.raises(ValueError):
            model.initialize_itinf(X, step=bad)
    for bad in (0.0, -0.5, float("nan"), float("inf"), [0.1], [0.1, -0.2]):
        for kw in (dict(step=2), dict(target_bpp=0.3), {}):
            with pytest.raises(ValueError, match="rd_lambda"):
                model.compress(X, itinf=dict(steps=2, rd_lambda=bad, **kw))
        with pytest.raises(ValueError, match="rd_lambda"):
            model.initialize_itinf(X, rd_lambda=bad)
    for bad in ([0.3], [0.1, 0.2, 0.3], float("inf")):
        with pytest.raises(ValueError, match="target_bpp"):
            model.compress(X, itinf=dict(steps=2, target_bpp=bad))
    # the exclusion at the top level stays
    with pytest.raises(ValueError, match="itinf"):
        model.compress(X, itinf=dict(steps=2, step=1), step=1)
    fact = stand_in(factorized=True)
    for kw in (dict(step=1), dict(step=0), dict(target_bpp=0.3), dict(rd_lambda=0.1)):
        with pytest.raises(NotImplementedError, match="hyperprior"):
            fact.compress(X, itinf=dict(steps=2, **kw))
    with pytest.raises(NotImplementedError, match="hyperprior"):
        fact.initialize_itinf(X, step=1)
    split = stand_in(_precision="bf16x3")
    for kw in (dict(step=1), dict(target_bpp=0.3)):
        with pytest.raises(NotImplementedError, match="fp32"):
            split.compress(X, itinf=dict(steps=2, **kw))
    with pytest.raises(NotImplementedError, match="fp32"):
        split.initialize_itinf(X, step=1)
    with pytest.raises(TypeError):                                 # an unknown key is still an error
        model.compress(X, itinf=dict(steps=2, stepp=1))


def test_step_mode_quant_record():
    """Every index 0 and no rd_lambda is the path of before (None); anything else records the indexes and each image's lambda."""
    model = stand_in()
    assert model._itinf_grid_of(X.shape, None, None, None) is None
    assert model._itinf_grid_of(X.shape, 0, None, None) is None and model._itinf_grid_of(X.shape, [0, 0], None, None) is None
    q = model._itinf_grid_of(X.shape, [0, 6], None, None)
    from shallow_ntc_amd import entropy_coding as ec
    assert q["grid"].kind == "image" and q["grid"].steps == [0, 6] and q["lam"].tolist() == [0.02, 0.02 / ec.step_size(6) ** 2]
    q = model._itinf_grid_of(X.shape, None, 0.5, None)                # a lambda per image keeps the per-image kernels at step 0
    assert q["grid"].kind == "image" and q["grid"].steps == [0, 0] and q["lam"].tolist() == [0.5, 0.5]
