"""Rate-distortion optimised quantisation, host side (no GPU): the argument checks of ``compress(x, rdoq=...)`` /
``coded_cost(x, rdoq=...)`` on a stand-in model (every refusal before anything reaches the device), the weight formula, the
ABI, and the invariants of the NumPy restatement the GPU tests hold the kernels to."""
from pathlib import Path

import numpy as np
import pytest

from test_hip_rdoq import np_rdoq
from test_rans_cost_host import np_cost, ref_cost_table

ROOT = Path(__file__).resolve().parent.parent
C = 8


class Launched(Exception):
    pass


def stand_in(**over):
    from shallow_ntc_amd.mshyper.models import Model

    class Stub:
        _latent_config = dict(uq=dict(method="sga"))
        _optimizer_config = {}
        _precision = "fp32"
        _distortion = "mse"
        _rd_lambda = 0.02
        _scheduled_rd_lambda = 0.02
        _bottleneck_size = C
        factorized = False
        compress = Model.compress
        coded_cost = Model.coded_cost
        _coded_cost = Model._coded_cost
        _compress_rdoq = Model._compress_rdoq
        _check_step_arguments = Model._check_step_arguments
        _check_rdoq_arguments = Model._check_rdoq_arguments
        _check_residual_arguments = Model._check_residual_arguments

        def _as_device_images(self, x):
            raise Launched

        def infer_latent_rvs(self, x):
            raise Launched

        def latent_gains(self):
            raise Launched

        def _get_codec(self):
            raise Launched

    stub = Stub()
    for k, v in over.items():
        setattr(stub, k, v)
    return stub


X = np.zeros((2, 64, 64, 3), np.float32)


def test_rdoq_refusals_come_before_any_launch():
    model = stand_in()
    for call in (model.compress, model.coded_cost):
        for ok in (True, {}, dict(strength=0.5), dict(zero=False), dict(gains=np.ones(C)), dict(gains=[0.0] * C, strength=2, zero=True)):
            with pytest.raises(Launched):                          # the stand-in works: a valid call reaches the device
                call(X, rdoq=ok)
            with pytest.raises(Launched):
                call(X, rdoq=ok, step=[1, -2], step_offsets=np.zeros((2, 4, 4), np.int8))
        with pytest.raises(Launched):                              # off: the call of before
            call(X, rdoq=None)
        for bad in (dict(strength=0), dict(strength=-2.0), dict(strength=float("nan")), dict(strength=float("inf")), dict(strength=None),
                    dict(gains=np.ones(C + 1)), dict(gains=np.ones((1, C))), dict(gains=[-1.0] + [1.0] * (C - 1)),
                    dict(gains=[float("inf")] * C), dict(gains="g"), dict(lam=0.1), 0.5, "on", [1]):
            with pytest.raises(ValueError):
                call(X, rdoq=bad)
    cfg = model._check_rdoq_arguments("compress", dict(gains=range(C)))
    assert cfg["strength"] == 1.0 and cfg["zero"] is True and cfg["gains"].dtype == np.float64 and cfg["gains"].tolist() == list(range(C))
    assert model._check_rdoq_arguments("compress", True) == dict(strength=1.0, zero=True, gains=None)
    assert model._check_rdoq_arguments("compress", None) is None and model._check_rdoq_arguments("compress", False) is None
    for kw in (dict(itinf=dict(steps=2)), dict(target_bpp=0.3), dict(target_psnr=33.0)):
        with pytest.raises(ValueError, match="rdoq excludes"):
            model.compress(X, rdoq=True, **kw)
    with pytest.raises(Launched):
        model.compress(X, rdoq=True, max_error=2)
    fact = stand_in(factorized=True)
    split = stand_in(_precision="bf16x3")
    ssim = stand_in(_distortion="ms_ssim")
    for stub, word in ((fact, "factorized"), (split, "bf16x3"), (ssim, "ms_ssim")):
        for call in (stub.compress, stub.coded_cost):
            with pytest.raises(NotImplementedError, match=word):
                call(X, rdoq=True)


def test_weight_formula():
    from shallow_ntc_amd import entropy_coding as ec
    g = np.array([0.0, 1.0, 3.0, 1234.5, 1e30], np.float64)
    w = ec.rdoq_weights(0.02, g)
    assert w.dtype == np.float32 and w.tolist() == (65536.0 * 0.02 * g / 3.0).astype(np.float32).tolist()
    assert ec.rdoq_weights(0.02, g, 0.25).tolist() == (0.25 * 65536.0 * 0.02 * g / 3.0).astype(np.float32).tolist()
    assert ec.rdoq_weights(1.0, [3.0], 1.0).tolist() == [65536.0] and ec.COST_UNIT == 65536
    # in cost_q units J H W = cost_q + 65536 lam SSE / 3, and an error of e symbol units in channel c at step s moves the SSE by
    # g_c (e s)^2; with lam_i = lam / s^2 the step cancels: the weight of e^2 is 65536 lam g_c / 3 at every step
    lam, s, e, gc, hw = 0.02, ec.step_size(7), 0.37, 55.0, 4096.0
    j_units = 65536.0 * hw * ((lam / s ** 2) * gc * (e * s) ** 2 / (3.0 * hw))
    assert abs(j_units - float(ec.rdoq_weights(lam, [gc])[0]) * e * e) <= 1e-6 * j_units
    for bad in (dict(lam=0.0), dict(lam=float("nan")), dict(strength=0.0), dict(strength=float("inf")), dict(gains=[]), dict(gains=[[1.0]]),
                dict(gains=[-1e-9]), dict(gains=[float("nan")])):
        kw = dict(lam=0.02, gains=[1.0], strength=1.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            ec.rdoq_weights(**kw)
    assert ec.check_enable(None, 3) == [1, 1, 1] and ec.check_enable([True, 0, np.int32(1)], 3) == [1, 0, 1]
    for bad in ([1], [1, 2, 0], [0.5, 1, 1], "110"):
        with pytest.raises(ValueError):
            ec.check_enable(bad, 3)
    tool = ec.Rdoq(w, 2, tables=None, zero=False)
    assert tool.flags == 0 and tool.enable == [1, 1] and ec.Rdoq(w, 2, None).flags == ec.RDOQ_TRY_ZERO == 1
    assert tool.set_enable([0, 1]) is tool and tool.enable == [0, 1]


def test_abi_and_build():
    import re
    from shallow_ntc_amd import _capi
    lib = _capi.load()
    header = (ROOT / "include" / "sntc.h").read_text()
    for name in ("sntc_rdoq_symbols", "sntc_rdoq_map_symbols"):
        assert name in _capi.SIGNATURES and hasattr(lib, name) and re.search(rf"\bint {name}\(", header)
        assert _capi.SIGNATURES[name][1][-1] is _capi.C.c_void_p and len(_capi.SIGNATURES[name][1]) == 20
    csrc = ROOT / "shallow-ntc_amd" / "csrc"
    make = (csrc / "Makefile").read_text()
    assert "rdoq.hip" in make and "rdoq_rules.h" in make
    # one copy of the decision: the kernel file takes it from the header
    kernel, rules = (csrc / "rdoq.hip").read_text(), (csrc / "rdoq_rules.h").read_text()
    assert '#include "rdoq_rules.h"' in kernel and "rdoq_choose(" in kernel and "__fadd_rn" not in kernel
    assert rules.count("__fadd_rn") == 1 and "fmaf" not in rules


def synthetic(seed, n=3, hw=700, c=C):
    from shallow_ntc_amd import entropy_coding as ec
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, 64, size=(n, hw, c)).astype(np.int16)
    mu = (rng.standard_normal((n, hw, c)) * 2).astype(np.float32)
    sig = 0.11 * np.exp(ec.SCALE_FACTOR * ids.astype(np.float64))
    y = (mu + rng.standard_normal((n, hw, c)) * sig * np.where(rng.random((n, hw, c)) < 0.2, 4.0, 1.0)).astype(np.float32)
    y.reshape(n, -1)[:, :6] = [np.nan, np.inf, -np.inf, 1e9, -1e9, 0.0]
    return y, mu, ids


@pytest.mark.parametrize("flags", [0, 1])
def test_the_restatement_never_raises_the_bits_and_keeps_s0_on_ties(flags):
    from shallow_ntc_amd import entropy_coding as ec
    tabs = ec.normal_tables()
    q = ref_cost_table(tabs)
    rng = np.random.default_rng(3)
    for seed, ks in ((0, [0, 0, 0]), (1, [-32, 5, 32]), (2, [-4, 2, 9])):
        y, mu, ids = synthetic(seed)
        n, hw, c = y.shape
        for k in (np.array(ks).reshape(n, 1, 1), rng.integers(-40, 41, size=(n, hw, 1))):
            for w in (np.zeros(c, np.float32), (rng.uniform(0.01, 5.0, c) * 65536).astype(np.float32), np.full(c, 1e30, np.float32)):
                sym, tid, changed, s0 = np_rdoq(y, mu, ids, k, w, [1, 1, 0], flags, tabs, q)
                plain = np_rdoq(y, mu, ids, k, w, [0, 0, 0], flags, tabs, q)
                assert (plain[0] == s0).all() and (plain[1] == tid).all() and plain[2].tolist() == [0] * n
                cost, cost0 = np_cost(sym.reshape(n, -1), tid.reshape(n, -1), tabs, q), np_cost(s0.reshape(n, -1), tid.reshape(n, -1), tabs, q)
                for i in range(n):
                    assert cost[i] <= cost0[i] and (cost[i] < cost0[i]) == (changed[i] > 0)
                assert changed[2] == 0 and (sym[2] == s0[2]).all()
                sym, s0 = sym.astype(np.int64), s0.astype(np.int64)                # |INT_MIN| needs the room
                moved = sym != s0
                assert (np.abs(sym[moved]) < np.abs(s0[moved])).all() and (s0[moved] != 0).all()
                if not flags:
                    assert (np.abs(s0[moved] - sym[moved]) == 1).all()
                assert (sym.reshape(n, -1)[:, 0] == 0).all()                       # NaN: symbol 0, never moved
                if w[0] == 0:
                    assert changed[0] > 0 and changed[1] > 0
                if w[0] >= 1e30:
                    assert changed.tolist() == [0] * n
    # equal J keeps the earlier candidate: u on a .5 tie with a flat price (weight 0, a table whose two entries cost the same)
    flat = [(0, np.array([16384, 16384, 16384, 16384], np.int64))] * 64
    qf = ref_cost_table(flat)
    y = np.array([[[0.5, 1.5, 2.5, -1.5, 1.2, 1.0, -2.5, 2.0]]], np.float32)
    sym, _, changed, s0 = np_rdoq(y, np.zeros_like(y), np.zeros(y.shape, np.int16), np.zeros((1, 1, 1), np.int64), np.zeros(8), [1], 1, flat, qf)
    assert s0.reshape(-1).tolist() == [0, 2, 2, -2, 1, 1, -2, 2]
    assert sym.reshape(-1).tolist() == [0, 2, 2, 0, 1, 1, 0, 2] and changed.tolist() == [2]
    # (symbols 0 .. 2 cost the same: s0 stays; -2 and -1 escape, 16 bits dearer than 0, which a = -1 does not beat but 0 does)
    sym = np_rdoq(y, np.zeros_like(y), np.zeros(y.shape, np.int16), np.zeros((1, 1, 1), np.int64), np.zeros(8), [1], 0, flat, qf)[0]
    assert sym.reshape(-1).tolist() == [0, 2, 2, -2, 1, 1, -2, 2]
