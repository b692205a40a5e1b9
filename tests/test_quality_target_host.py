"""Host half of quality-targeted compress ("quality target"): the selection rule ``select_quality`` on hand-made
rows, the checks of ``target_psnr``, and the refusals of ``compress(x, target_psnr=...)`` -- every one of them before anything is
launched.  No GPU: the model is a stand-in whose first device call raises (the pattern of test_sga_step_host.py)."""
import math
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
ENTRY_POINTS = ("sntc_step_ladder_dequant", "sntc_step_map_ladder_dequant")


def test_entry_points_declared_bound_and_built():
    from shallow_ntc_amd import _capi
    header = (ROOT / "include" / "sntc.h").read_text()
    lib = _capi.load()
    for name in ENTRY_POINTS:
        assert re.search(rf"\bint {name}\(", header), f"{name} is not declared in include/sntc.h"
        assert name in _capi.SIGNATURES and hasattr(lib, name)
        assert _capi.SIGNATURES[name][1][-1] is _capi.C.c_void_p          # the stream comes last
    assert "quant_step.hip" in (ROOT / "shallow-ntc_amd" / "csrc" / "Makefile").read_text()
    text = (ROOT / "shallow-ntc_amd" / "csrc" / "quant_step.hip").read_text()
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    # one copy of the step rule, and the shape the kernel promises: no atomics, no LDS
    assert '#include "step_rules.h"' in code and "float step_diff(" not in code and "rintf" not in code and "fmaf" not in code
    kernel = code.split("void __launch_bounds__(kDequantLadderThreads) step_ladder_dequant_kernel(")
    assert len(kernel) == 2                                      # one body for the per-image and the map candidates
    body = kernel[1].split("\n}\n")[0]
    assert "step_value(step_round(" in body and "atomic" not in body and "__shared__" not in body and "__syncthreads" not in body


def test_select_quality_takes_the_cheapest_candidate_that_qualifies():
    from shallow_ntc_amd import entropy_coding as ec
    steps = [-2, -1, 0, 1, 2]
    # image 0: bits are not monotone -- index 0 is cheaper than the coarser index 1, and both qualify: 0 wins, not the coarsest
    # image 1: sse is not monotone -- index 2 misses the budget although index 1 and the finer ones meet it; 1 is cheapest
    bits = [[900.0, 800.0, 500.0, 600.0, 300.0], [900.0, 800.0, 700.0, 650.0, 300.0]]
    sse = [[10, 20, 30, 40, 500], [10, 20, 30, 25, 60]]
    rows = ec.select_quality(bits, sse, [45.0, 29.0], steps, elements=3 * 8 * 8)
    assert [r["step_chosen"] for r in rows] == [0, 1]
    assert rows[0] == dict(step_chosen=0, bits_predicted=500.0, sse_predicted=30.0, sse_budget=45.0, met=True,
                           psnr_predicted=10.0 * math.log10(255.0 ** 2 * 192 / 30.0))
    assert rows[1]["bits_predicted"] == 650.0 and rows[1]["sse_predicted"] == 25.0 and rows[1]["met"] is True
    # without the pixel count there is no PSNR to report
    assert ec.select_quality(bits, sse, [45.0, 29.0], steps)[0]["psnr_predicted"] is None
    # the candidates need not be sorted, nor be the whole ladder
    rows = ec.select_quality([[300.0, 500.0, 900.0]], [[500, 30, 10]], [45.0], [2, 0, -2])
    assert rows[0]["step_chosen"] == 0 and rows[0]["bits_predicted"] == 500.0


def test_select_quality_on_equal_bits_takes_the_larger_index():
    from shallow_ntc_amd import entropy_coding as ec
    rows = ec.select_quality([[400.0, 300.0, 300.0, 300.0]], [[1, 2, 3, 99]], [50.0], [-3, 4, 9, 12])
    assert rows[0]["step_chosen"] == 9 and rows[0]["sse_predicted"] == 3.0            # 12 has the same bits but misses
    rows = ec.select_quality([[300.0, 300.0]], [[3, 2]], [50.0], [9, 4])                # whatever the order they come in
    assert rows[0]["step_chosen"] == 9


def test_select_quality_where_nothing_qualifies():
    from shallow_ntc_amd import entropy_coding as ec
    ladder = list(range(ec.STEP_MIN, ec.STEP_MAX + 1))
    bits = np.linspace(9000.0, 1000.0, len(ladder))[None]
    sse = np.linspace(100.0, 9000.0, len(ladder))[None]
    row = ec.select_quality(bits, sse, [99.0], ladder)[0]
    assert row["step_chosen"] == ec.STEP_MIN and row["met"] is False
    assert row["bits_predicted"] == 9000.0 and row["sse_predicted"] == 100.0 and row["sse_budget"] == 99.0
    # candidates that do not hold STEP_MIN: the step is still STEP_MIN, and nothing is predicted for it
    row = ec.select_quality([[5.0, 4.0]], [[100, 200]], [99.0], [0, 1])[0]
    assert row["step_chosen"] == ec.STEP_MIN and row["met"] is False and math.isnan(row["bits_predicted"]) and math.isnan(row["sse_predicted"])


def test_select_quality_at_the_budget_boundary():
    """The budget is a float64, the SSE an integer: sse == floor(budget) qualifies, one more does not."""
    from shallow_ntc_amd import entropy_coding as ec
    H, W = 200, 120
    budget = ec.quality_budgets(ec.check_quality(31.7, 1), H, W)
    assert budget.dtype == np.float64 and abs(budget[0] / (255.0 ** 2 * 3 * H * W / 10.0 ** (31.7 / 10.0)) - 1.0) < 1e-15    # one ulp of pow
    at = math.floor(budget[0])
    assert at < budget[0]                                                              # not an integer: the floor is the last fit
    for sse, want, met in ((at, 5, True), (at + 1, ec.STEP_MIN, False)):
        row = ec.select_quality([[900.0, 100.0]], [[sse + 7, sse]], budget, [ec.STEP_MIN, 5], elements=3 * H * W)[0]
        assert row["step_chosen"] == want and row["met"] is met
    assert row["psnr_predicted"] < 31.7                                                # what STEP_MIN gives is reported, not the target
    assert ec.psnr_of_sse(at, 3 * H * W) >= 31.7 > ec.psnr_of_sse(at + 1, 3 * H * W)
    assert ec.psnr_of_sse(0, 12) == np.inf
    # per-image targets give per-image budgets; a higher target is a smaller budget
    b = ec.quality_budgets(ec.check_quality([30.0, 40.0], 2), 64, 64)
    assert b[0] == 255.0 ** 2 * 3 * 64 * 64 / 1000.0 and b[1] == 255.0 ** 2 * 3 * 64 * 64 / 10000.0


def test_select_quality_shape_errors():
    from shallow_ntc_amd import entropy_coding as ec
    good = dict(bits=[[1.0, 2.0], [1.0, 2.0]], sse=[[1, 2], [1, 2]], sse_budget=[5.0, 5.0], steps=[0, 1])
    assert len(ec.select_quality(**good)) == 2
    for bad in (dict(bits=[1.0, 2.0]), dict(sse=[[1, 2]]), dict(sse=[[1, 2, 3], [1, 2, 3]]), dict(sse_budget=[5.0]),
                dict(steps=[0, 1, 2]), dict(bits=[[1.0], [1.0]])):
        with pytest.raises(ValueError, match="select_quality"):
            ec.select_quality(**{**good, **bad})


def test_check_quality():
    from shallow_ntc_amd import entropy_coding as ec
    assert ec.check_quality(32, 3).tolist() == [32.0] * 3 and ec.check_quality(np.float32(30.5), 1).tolist() == [30.5]
    assert ec.check_quality([30.0, 41.5], 2).tolist() == [30.0, 41.5]
    for bad in (float("nan"), float("inf"), [30.0], [30.0, 31.0, 32.0], [30.0, float("nan")], [[30.0, 31.0]], "high", None):
        with pytest.raises(ValueError, match="target_psnr"):
            ec.check_quality(bad, 2)


class Launched(Exception):
    pass


def stand_in(**over):
    """What ``compress`` reads before it touches the device; the first device call raises."""
    from shallow_ntc_amd.mshyper.models import Model

    class Stub:
        _latent_config = dict(uq=dict(method="sga"))
        _optimizer_config = {}
        _precision = "fp32"
        _distortion = "mse"
        _rd_lambda = 0.02
        factorized = False
        compress = Model.compress
        rd_curve = Model.rd_curve
        _check_step_arguments = Model._check_step_arguments
        _compress_itinf = Model._compress_itinf

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


def test_target_psnr_refusals_come_before_any_launch():
    model = stand_in()
    with pytest.raises(Launched):                                  # the stand-in works: a valid call reaches the device
        model.compress(X, target_psnr=33.0)
    with pytest.raises(Launched):
        model.compress(X, target_psnr=[33.0, 35.0], step_offsets=np.zeros((2, 4, 4), np.int8))
    with pytest.raises(Launched):
        model.rd_curve(X)
    # positional callers of before keep working, and the new keyword is the trailing one
    assert model._check_step_arguments("compress", None) is None
    assert model._check_step_arguments("compress", None, None, None, None) is None
    assert model._check_step_arguments("compress", 1, None, None, None) is None
    assert model._check_step_arguments("compress", None, target_psnr=30.0) is None
    for kw in (dict(step=1), dict(target_bpp=0.3), dict(step=0), dict(step=1, target_bpp=0.3)):
        with pytest.raises(ValueError, match="exclude"):
            model.compress(X, target_psnr=33.0, **kw)
    with pytest.raises(ValueError, match="itinf"):
        model.compress(X, target_psnr=33.0, itinf=dict(steps=2))
    with pytest.raises(ValueError, match="not implemented inside itinf"):
        model.compress(X, itinf=dict(steps=2, target_psnr=33.0))
    fact = stand_in(factorized=True)
    with pytest.raises(NotImplementedError, match="factorized"):
        fact.compress(X, target_psnr=33.0)
    with pytest.raises(NotImplementedError, match="factorized"):
        fact.rd_curve(X)
    split = stand_in(_precision="bf16x3")
    with pytest.raises(NotImplementedError, match="bf16x3"):
        split.compress(X, target_psnr=33.0)
    with pytest.raises(NotImplementedError, match="bf16x3"):
        split.rd_curve(X, steps=[0, 1])
    for bad in ([40], [1, 33], [1.5], []):
        with pytest.raises(ValueError):
            model.rd_curve(X, steps=bad)
