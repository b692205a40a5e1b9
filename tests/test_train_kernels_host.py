"""What tests/test_hip_train_kernels.py relies on, checked without a GPU: the inputs hold what the kernels' branches switch on,
no reference gradient is identically zero, the split-K and slab geometry of the case tables is what csrc/wgrad.hip computes, and
the float64 reference of every backward kernel agrees with central finite differences of its forward restatement."""
import math

import numpy as np
import pytest
import torch

import train_kernel_cases as K
from oracle import train_ref
from train_kernel_cases import SGA_CAP, TR_CAP, f64


def _fd(fn, x, at, eps=1e-6):
    """Central finite differences of the scalar fn at the flat indices ``at`` of the float64 array x."""
    out = []
    for i in at:
        hi, lo = x.copy(), x.copy()
        hi.reshape(-1)[i] += eps
        lo.reshape(-1)[i] -= eps
        out.append((fn(hi) - fn(lo)) / (2 * eps))
    return np.array(out)


def _close(fd, ref, tol=1e-7):
    assert np.abs(fd - ref).max() <= tol * max(1.0, np.abs(ref).max()), (fd, ref)


# ---- preconditions ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("total", K.EW_SIZES)
def test_elementwise_inputs_hold_what_the_branches_switch_on(total):
    d = K.elementwise_inputs(total)
    assert all(v.size == total and v.dtype == np.float32 for v in d.values())
    assert (d["norm"] > 0).all() and (0 < d["s"]).all() and (d["s"] < 1).all() and (np.abs(d["noise"]) <= 0.5).all()
    if total > 1000:
        assert total > 2 * TR_CAP > 2 * SGA_CAP and total % 4 == 3
    if total >= 255:
        for k in ("x", "y"):
            assert min(K.count_zeros(d[k])) >= 64
        cls = K.reparam_classes(d["raw"], d["g_eff"])
        assert cls["at_bound"] >= 8 and min(cls["below_neg"], cls["below_pos"], cls["above_neg"], cls["above_pos"]) >= (64 if total > 1000 else 48), cls
    if total > 1000:                                          # zeros and every class in the last trip as well
        last = slice(2 * TR_CAP, None)
        assert (d["raw"][last] < K.GDN_BOUND).any() and (d["raw"][last] >= K.GDN_BOUND).any()
    assert float(K.GDN_BOUND) == pytest.approx(math.sqrt(1e-6 + 2.0 ** -36)) and float(K.GDN_PEDESTAL) == 2.0 ** -36


def test_grid_caps_are_the_ones_in_the_sources():
    from pathlib import Path
    csrc = Path(__file__).resolve().parent.parent / "shallow-ntc_amd" / "csrc"
    assert "b > 2048 ? 2048 : b" in (csrc / "train.hip").read_text() and TR_CAP == 2048 * 256
    sga = (csrc / "sga.hip").read_text()
    assert "b > 1024 ? 1024 : b" in sga and "dim3(grid_for(npix)), dim3(256)" in sga and SGA_CAP == 1024 * 256
    assert "std::min(tr_grid(total), 1024)" in (csrc / "train.hip").read_text()
    assert K.TRANSPOSE_CASES[-1][0] * K.TRANSPOSE_CASES[-1][1] * K.TRANSPOSE_CASES[-1][2] > 2 * TR_CAP
    assert K.MATMUL_CASES[0][2] > TR_CAP and K.ADAM_N > 2 * SGA_CAP
    rows, k, _ = K.MATMUL_CASES[-1]
    assert rows * k * 4 == 48 * 1024 and K.MATMUL_REFUSED[0] * K.MATMUL_REFUSED[1] * 4 > 48 * 1024


@pytest.mark.parametrize("ch,has_res", [(ch, r) for ch in (12, 24, 48) for r in (0, 1)])
def test_tail_inputs_and_references(ch, has_res):
    d = K.tail_inputs(ch, has_res, K.TAIL_NPIX)
    assert min(K.count_zeros(d["t"][:, :ch])) >= 64 and (d["beta"] >= 1e-3).all() and (d["gamma"] >= 0).all()
    zero = d["t"][:, :ch] == 0
    refs = {act: K.tail_reference(ch, has_res, act, K.TAIL_NPIX) for act in (0, 1, 2, 3, 4)}
    for act, ref in refs.items():
        assert np.abs(ref["g_t"]).max() > 0 and np.abs(ref["h"]).max() > 0
        if has_res:
            assert np.array_equal(ref["g_t"][:, ch:], f64(d["g_h"]))
    g = f64(d["g_h"])
    assert (refs[3]["g_t"][:, :ch][zero] == 0).all()                                  # relu: nothing through a zero of either sign
    assert np.array_equal(refs[4]["g_t"][:, :ch][zero], 0.2 * g[zero]) and (g[zero] != 0).all()      # leaky_relu: 0.2, not 1
    assert np.array_equal(refs[0]["g_t"][:, :ch], g)
    assert np.array_equal(refs[1]["g_t"][:, :ch][zero], (g * (f64(d["beta"]) + np.abs(f64(d["t"][:, :ch])) @ f64(d["gamma"])))[zero])


def test_adam_inputs_and_reference():
    d = K.adam_inputs()
    still = d["still"]
    assert len(still) == 64 and not (d["g"][still].any() or d["m"][still].any() or d["v"][still].any())
    moving = np.setdiff1d(np.arange(K.ADAM_N), still)
    assert (d["m"][moving] != 0).all() and (d["v"] >= 0).all() and (d["v"][moving] > 0).all()
    for t in K.ADAM_STEPS:
        p1 = K.adam_reference(t)["p"][0]
        assert np.array_equal(p1[still], f64(d["p"])[still]) and np.isfinite(p1).all() and (p1[moving] != f64(d["p"])[moving]).any()


# ---- geometry of the slab tables ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,expect", K.WG_CASES, ids=K.WG_IDS)
def test_wgrad_case_geometry(case, expect):
    from shallow_ntc_amd import _capi as capi
    kind, k, s, cin, cout, n, h, w = case
    geo = K.wg_split(*case)
    assert (geo["P"], geo["ksplit"], geo["last_slab"], geo["last_stage"]) == expect
    nbytes = capi.load().sntc_conv_wgrad_workspace_bytes(K.WG_KINDS[kind], k, k, s, cin, cout, n, h, w)
    assert nbytes == (4 * geo["ksplit"] * geo["M"] * geo["N"] if geo["ksplit"] > 1 else 0)
    assert n >= 2 and K.wg_stages_straddle(geo) and geo["Cd"] % 4 == 0
    assert (K.WG_KINDS["conv"], K.WG_KINDS["convT"], K.WG_KINDS["sigdown"], K.WG_KINDS["sigup"]) == \
        (capi.CONV2D, capi.CONV2D_TRANSPOSE, capi.SIGNAL_DOWN, capi.SIGNAL_UP)
    if kind in ("conv", "sigdown") and s > 1:                           # an odd input: Hs is not stride * Hd, SAME pads unevenly
        assert h != s * geo["Hd"] and w != s * geo["Wd"]


@pytest.mark.parametrize("shape,slabs", K.BIAS_CASES)
def test_bias_case_geometry(shape, slabs):
    from shallow_ntc_amd import _capi as capi
    npix, c = shape
    assert K.bias_slabs(npix, c) == slabs and capi.load().sntc_bias_grad_workspace_bytes(npix, c) == 4 * slabs * c
    ref = K.bias_case(npix, c)["ref"]
    assert ref.shape == (c,) and np.abs(ref).min() > 0


def test_prior_case_geometry():
    """factorized_param_grad_kernel: 64-channel strips x min(256, ceil(npix / 4)) pixel slabs of ceil(npix / slabs) pixels."""
    seen = set()
    for c, n, hw in K.PRIOR_CASES:
        npix = n * hw
        slabs = min(256, (npix + 3) // 4)
        per = -(-npix // slabs)
        seen.add((c % 64 != 0, npix < 4, slabs == 256 and npix % per != 0))
    assert {(c, n * hw) for c, n, hw in K.PRIOR_CASES} == {(c, p) for c in (32, 100, 192) for p in (3, 1026)} | {(192, 1400)}
    assert any(s[0] for s in seen) and any(s[1] for s in seen) and any(s[2] for s in seen)


# ---- the references against finite differences ------------------------------------------------------------------------------
def test_elementwise_backward_references_against_finite_differences():
    rng = np.random.default_rng(5)
    u, g, t = (rng.standard_normal((5, 8)) for _ in range(3))                # 5 pixels, 8 channels, no zeros
    at = range(0, 40, 3)
    for act in ("none", "relu", "leaky_relu", "sigmoid"):
        fwd = lambda v: train_ref.ACTIVATIONS[act](torch.from_numpy(v)).numpy()
        ref = K.act_backward_ref(g, fwd(u), act)[0]
        _close(_fd(lambda v: float((g * fwd(v)).sum()), u, at), ref.reshape(-1)[list(at)])
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    spre, x = rng.standard_normal((5, 8)), rng.standard_normal((5, 8))
    gate = lambda tt, sp: float((g * K.gate_forward_ref(x, tt, sig(sp))[0]).sum())
    (g_t, _, _), (g_s, _, _) = K.gate_backward_ref(g, t, sig(spre))
    _close(_fd(lambda v: gate(v, spre), t, at), g_t.reshape(-1)[list(at)])
    _close(_fd(lambda v: gate(t, v), spre, at), g_s.reshape(-1)[list(at)])
    # GDN1 / IGDN1 through the three element-wise kernels and the 1x1 contractions between them, against train_ref.gdn
    beta, gamma = 1.0 + 0.5 * rng.random(8), 0.1 * np.eye(8) + 0.02 * rng.random((8, 8))
    for inverse in (0, 1):
        def layer(v):
            y = train_ref.gdn(torch.from_numpy(v.T.reshape(1, 8, 5, 1)), torch.from_numpy(beta), torch.from_numpy(gamma), inverse=bool(inverse))
            return y.reshape(8, 5).t().numpy()
        norm = beta + np.abs(u) @ gamma
        assert np.allclose(K.gdn_apply_ref(u, norm, inverse)[0], layer(u), rtol=1e-13)
        (q, _, _), ax = K.gdn_prep_ref(g, u, norm, inverse)
        dx = K.gdn_finish_ref(g, u, norm, q @ gamma.T, inverse)[0]             # t = q gamma^T: the adjoint 1x1 plan
        _close(_fd(lambda v: float((g * layer(v)).sum()), u, at), dx.reshape(-1)[list(at)])
        _close(_fd(lambda b: float((g * (u * (b + ax @ gamma) if inverse else u / (b + ax @ gamma))).sum()), beta, range(8)), q.sum(0))
    # the reparameterisation: a true derivative above the bound; below it the rule passes what pushes raw up and nothing else
    raw = np.array([0.5, 0.03, 0.9, float(K.GDN_BOUND) / 2, float(K.GDN_BOUND) / 4])
    g_eff = np.array([1.5, -0.7, 0.2, 0.8, -0.6])
    ref = K.reparam_backward_ref(raw, g_eff)[0]
    fd = _fd(lambda v: float((g_eff * K.reparam_forward_ref(v)[0]).sum()), raw, range(5), eps=1e-5)
    _close(fd[:4], ref[:4])
    assert fd[3] == 0 and fd[4] == 0 and ref[3] == 0 and ref[4] == g_eff[4] * 2 * float(K.GDN_BOUND)


@pytest.mark.parametrize("act", [0, 1, 2, 3, 4])
def test_tail_reference_against_finite_differences(act):
    ch, has_res, npix = 12, 1, K.TAIL_NPIX
    d, ref = K.tail_inputs(ch, has_res, npix), K.tail_reference(ch, has_res, act, npix)
    keep = np.flatnonzero((d["t"] != 0).all(axis=1))[:5]                    # 5 pixels without a kink
    t, g = f64(d["t"])[keep], f64(d["g_h"])[keep]
    beta, gamma = torch.tensor(f64(d["beta"])), torch.tensor(f64(d["gamma"]))
    fn = lambda v: float((K.hidden_forward(torch.from_numpy(v), ch, has_res, act, beta, gamma).numpy() * g).sum())
    at = range(0, t.size, 7)
    _close(_fd(fn, t, at), ref["g_t"][keep].reshape(-1)[list(at)])


@pytest.mark.parametrize("case", [c for c, _ in K.WG_CASES], ids=K.WG_IDS)
def test_wgrad_reference_against_finite_differences(case):
    kind, k, s, cin, cout, n, h, w = case
    c = K.wg_case(case)
    assert np.abs(c["dw"]).min() > 0 and (c["S"] >= np.abs(c["dw"])).all()
    x, g = train_ref.as_input(c["x"]), train_ref.as_input(c["g"])
    rng = np.random.default_rng(1)
    at = sorted({0, c["dw"].size - 1, int(rng.integers(c["dw"].size))})         # first and last tap, one in between
    fn = lambda wv: float((K.wg_forward(kind, x, torch.from_numpy(wv), s) * g).sum())
    _close(_fd(fn, np.zeros(c["shape"]), at, eps=0.5), c["dw"].reshape(-1)[at], tol=1e-10)     # linear in w: exact at any step


def test_prior_reference_against_finite_differences():
    mats, biases, factors = K.prior_params(32)
    for c, n, hw in K.PRIOR_CASES:
        ref = K.prior_case(c, n, hw)
        assert all(np.abs(ref[k]).max() > 0 for k in ("dz", "gm", "gb", "gf")) and (ref["bits"] > 0).all()
    z = f64(K.prior_case(32, 2, 513)["z"])[0, :5]                          # 5 pixels
    T = lambda grp: [torch.tensor(f64(a)) for a in grp]

    def bits(zv=z, m=mats, b=biases, f=factors):
        return float(K.prior_bits(torch.from_numpy(zv), T(m), T(b), T(f)).sum())

    zt = torch.tensor(z, requires_grad=True)
    leaves = [[torch.tensor(f64(a), requires_grad=True) for a in grp] for grp in (mats, biases, factors)]
    K.prior_bits(zt, *leaves).sum().backward()
    at = range(0, z.size, 17)
    _close(_fd(bits, z, at), zt.grad.numpy().reshape(-1)[list(at)], tol=1e-6)
    for gi, grp in enumerate((mats, biases, factors)):
        for li, a in enumerate(grp):
            def fn(v):
                new = [f64(q) for q in grp]
                new[li] = v
                return bits(**{("m", "b", "f")[gi]: new})
            idx = range(0, a.size, max(1, a.size // 4))
            _close(_fd(fn, f64(a).copy(), idx), leaves[gi][li].grad.numpy().reshape(-1)[list(idx)], tol=1e-6)
