"""The training step's small kernels (csrc/train.hip, csrc/wgrad.hip, the backward half of csrc/sga.hip), one entry point at a
time against float64: past the caps of their grid-stride loops, at ragged slabs and strips, and on inputs that hold what
their branches switch on.  Cases, inputs, references and the derivation of every bar: tests/train_kernel_cases.py.

Measured on an MI355X, worst |got - ref| / (r 2^-24 S) over all cases (the bar is 1): element-wise kernels 1.00 at r = 1
(one rounding, at its half-ulp limit) and 0.81 - 0.96 at r = 2 .. 4; two_layer_hidden 1.00 (none / relu + residual, r = 1), 0.72 leaky_relu,
0.51 IGDN1, 0.43 GDN1; two_layer_tail_bwd 0.60 leaky_relu, 0.43 IGDN1, 0.15 GDN1; small_matmul 0.22; Adam 0.80; conv_wgrad 0.012 and bias_grad 0.0002 of the K = P bar,
6.7e-7 and 1.6e-7 of max|ref| (bar 2e-5); prior gradients 4.7e-6 of max|ref| (bar 2e-5); sumsq 7e-10 absolute on 1.05e6."""
import numpy as np
import pytest
import torch

import __graft_entry__ as graft

graft.load_package()
pytestmark = pytest.mark.gpu

import train_kernel_cases as K  # noqa: E402
from train_kernel_cases import SGA_CAP, TR_CAP  # noqa: E402


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _within(got, ref_r_S, what):
    """|got - ref| <= r 2^-24 S per element; r == 0: exact."""
    ref, r, S = ref_r_S
    got = got.cpu().numpy().reshape(np.shape(ref))
    if r == 0:
        assert np.array_equal(got, ref.astype(np.float32)), what
        return 0.0
    q = K.worst_ratio(got, ref, r, S)
    print(f"{what}: worst |got - ref| / (r 2^-24 S) = {q:.3f} at r = {r}")
    assert q <= 1.0, (what, q)
    return q


def _ew(total, dev, *names):
    d = K.elementwise_inputs(total)
    if total > 1000:
        assert total > 2 * TR_CAP and total % 4            # a third trip for some threads only; no whole float4 tail
    if total >= 255:
        for k in ("x", "y"):
            assert min(K.count_zeros(d[k])) >= 64
    assert (d["norm"] > 0).all()
    return d, [_dev(d[k], dev) for k in names]


# ---- 1. element-wise kernels of train.hip ------------------------------------------------------------------------------
@pytest.mark.parametrize("total", K.EW_SIZES)
def test_act_backward(total, dev):
    from shallow_ntc_amd import ops
    d, (g, y, s) = _ew(total, dev, "g", "y", "s")
    for act in ("none", "relu", "leaky_relu"):
        _within(ops.act_backward(g, y, act), K.act_backward_ref(d["g"], d["y"], act), act)
    _within(ops.act_backward(g, s, "sigmoid"), K.act_backward_ref(d["g"], d["s"], "sigmoid"), "sigmoid")


@pytest.mark.parametrize("total", K.EW_SIZES)
def test_gate_axpy_noise_tensor(total, dev):
    from shallow_ntc_amd import ops
    d, (g, x, t, s, b, noise) = _ew(total, dev, "g", "x", "t", "s", "b", "noise")
    _within(ops.gate_forward(x, t, s), K.gate_forward_ref(d["x"], d["t"], d["s"]), "gate_forward")
    g_t, g_s = ops.gate_backward(g, t, s)
    ref_t, ref_s = K.gate_backward_ref(d["g"], d["t"], d["s"])
    _within(g_t, ref_t, "gate_backward g_t")
    _within(g_s, ref_s, "gate_backward g_spre")
    alpha = float(np.float32(0.37))
    _within(ops.axpy(g.clone(), b, alpha), K.axpy_ref(d["g"], d["b"], alpha), "axpy")
    _within(ops.noise_add(x, noise), K.noise_add_ref(d["x"], d["noise"]), "noise_add")


def test_noise_add_generator_is_keyed_by_element(dev):
    from shallow_ntc_amd import ops
    total = 2 * TR_CAP + 259
    assert total > 2 * TR_CAP
    u = ops.noise_add(torch.zeros((total,), device=dev), None, seed=5, step=9).cpu().numpy()
    assert -0.5 < u.min() and u.max() < 0.5
    head = ops.noise_add(torch.zeros((1000,), device=dev), None, seed=5, step=9).cpu().numpy()
    assert np.array_equal(u[:1000], head)                    # the stream does not depend on the launch
    # a thread's second and third trip draw new values: 24-bit uniforms collide at 2^-24 per pair, i.e. 0.03 expected in 524,288
    for trip in (1, 2):
        a, b = u[trip * TR_CAP:(trip + 1) * TR_CAP], u[(trip - 1) * TR_CAP:trip * TR_CAP][:total - trip * TR_CAP]
        assert int((a == b[:a.size]).sum()) <= 8, trip


@pytest.mark.parametrize("total", K.EW_SIZES)
def test_sumsq(total, dev):
    from shallow_ntc_amd import ops
    d, (g,) = _ew(total, dev, "g")
    if total > 1000:
        assert total > 2 * SGA_CAP                           # sumsq launches at most 1024 blocks
    ref = float(np.sum(d["g"].astype(np.longdouble) ** 2))
    # the product of two float32 is exact in float64; each of the total additions (per thread, across lanes, the atomics)
    # rounds once in float64: r = total at 2^-53, S = the sum itself (all terms are non-negative)
    bar = total * 2.0 ** -53 * ref
    out = ops.sumsq(g)
    first = float(out.item())
    print(f"sumsq[{total}]: |got - ref| = {abs(first - ref):.3e}, bar {bar:.3e}")
    assert abs(first - ref) <= bar
    from shallow_ntc_amd import _capi as capi
    capi.call("sntc_sumsq", ops._ptr(g), total, ops._ptr(out), ops._stream())      # overwritten, not accumulated
    assert abs(float(out.item()) - ref) <= bar
    if total <= 256:                                         # one block: no atomics between blocks, the same bits
        assert float(out.item()) == first


@pytest.mark.parametrize("total", K.EW_SIZES)
def test_gdn_elementwise(total, dev):
    from shallow_ntc_amd import ops
    d, (g, x, norm, t) = _ew(total, dev, "g", "x", "norm", "t")
    for inverse in (0, 1):
        _within(ops.gdn_apply(x, norm, inverse), K.gdn_apply_ref(d["x"], d["norm"], inverse), f"gdn_apply[{inverse}]")
        q, ax = ops.gdn_backward_prep(g, x, norm, inverse)
        ref_q, ref_ax = K.gdn_prep_ref(d["g"], d["x"], d["norm"], inverse)
        _within(q, ref_q, f"gdn_backward_prep[{inverse}]")
        assert np.array_equal(ax.cpu().numpy(), ref_ax.astype(np.float32))
        assert not np.signbit(ax.cpu().numpy()).any()         # |-0.0| is +0.0
        _within(ops.gdn_backward_finish(g, x, norm, t, inverse), K.gdn_finish_ref(d["g"], d["x"], d["norm"], d["t"], inverse),
                f"gdn_backward_finish[{inverse}]")


@pytest.mark.parametrize("total", K.EW_SIZES)
def test_gdn_reparam(total, dev):
    from shallow_ntc_amd import _capi as capi, ops
    d, (raw, g_eff) = _ew(total, dev, "raw", "g_eff")
    if total >= 255:
        cls = K.reparam_classes(d["raw"], d["g_eff"])
        assert cls["at_bound"] >= 8 and min(cls["below_neg"], cls["below_pos"], cls["above_neg"], cls["above_pos"]) >= (64 if total > 1000 else 48), cls
    eff, g_raw = torch.empty_like(raw), torch.empty_like(raw)
    capi.call("sntc_gdn_reparam_forward", ops._ptr(raw), total, float(K.GDN_BOUND), float(K.GDN_PEDESTAL), ops._ptr(eff), ops._stream())
    _within(eff, K.reparam_forward_ref(d["raw"]), "gdn_reparam_forward")
    capi.call("sntc_gdn_reparam_backward", ops._ptr(raw), ops._ptr(g_eff), total, float(K.GDN_BOUND), ops._ptr(g_raw), ops._stream())
    ref = K.reparam_backward_ref(d["raw"], d["g_eff"])
    _within(g_raw, ref, "gdn_reparam_backward")
    blocked = (d["raw"] < K.GDN_BOUND) & (d["g_eff"] > 0)     # below the bound and pushed further down: no gradient
    got = g_raw.cpu().numpy()
    assert (got[blocked] == 0).all() and (got[~blocked] != 0).all()


@pytest.mark.parametrize("taps,a,b", K.TRANSPOSE_CASES)
def test_transpose_last2(taps, a, b, dev):
    from shallow_ntc_amd import ops
    if taps == 81:
        assert taps * a * b > 2 * TR_CAP
    src = np.arange(taps * a * b, dtype=np.float32).reshape(taps, a, b)          # every element its own value (< 2^24: exact)
    dst = torch.full((taps, b, a), -1.0, dtype=torch.float32, device=dev)
    ops.transpose_last2(_dev(src, dev), dst)
    assert np.array_equal(dst.cpu().numpy(), src.transpose(0, 2, 1))


# ---- 2. sntc_small_matmul ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transpose_a", [False, True])
@pytest.mark.parametrize("rows,k,cols", K.MATMUL_CASES)
def test_small_matmul(rows, k, cols, transpose_a, dev):
    from shallow_ntc_amd import ops
    if cols > 1031:
        assert cols > TR_CAP                                 # a second trip over the columns
    c = K.matmul_case(rows, k, cols, transpose_a)
    out = torch.full((rows, cols), 7.0, dtype=torch.float32, device=dev)
    ops.small_matmul(_dev(c["a"], dev), _dev(c["b"], dev), out, transpose_a=transpose_a)
    _within(out, (c["ref"], c["r"], c["S"]), f"small_matmul[{rows},{k},{cols},{int(transpose_a)}]")


def test_small_matmul_refuses_a_left_matrix_beyond_48_kb(dev):
    from shallow_ntc_amd import _capi as capi, ops
    rows, k, cols = K.MATMUL_REFUSED
    assert rows * k * 4 > 48 * 1024 >= (rows - 1) * k * 4
    a, b = torch.zeros((rows, k), device=dev), torch.zeros((k, cols), device=dev)
    with pytest.raises(capi.SntcError) as e:
        ops.small_matmul(a, b, torch.zeros((rows, cols), device=dev))
    assert e.value.code == capi.ERR_UNSUPPORTED


# ---- 3. sntc_two_layer_hidden, sntc_two_layer_tail_bwd --------------------------------------------------------------------
def _tail(ch, has_res, act, npix, dev):
    from shallow_ntc_amd import ops
    d, ref = K.tail_inputs(ch, has_res, npix), K.tail_reference(ch, has_res, act, npix)
    assert min(K.count_zeros(d["t"][:, :ch])) >= 64
    t, g_h = _dev(d["t"], dev).view(1, npix, 1, -1), _dev(d["g_h"], dev).view(1, npix, 1, ch)
    beta, gamma = _dev(d["beta"], dev), _dev(d["gamma"], dev)
    tag = f"[{ch},{has_res},{act},{npix}]"
    h = ops.two_layer_hidden(t, ch, has_res, act, beta, gamma)
    _within(h, (ref["h"],) + ref["fwd"], "two_layer_hidden" + tag)
    c2 = ch * (1 + has_res)
    for cp in (c2, c2 + 8):
        g_t, ax, gx = ops.two_layer_tail_bwd(t, g_h, ch, has_res, act, beta, gamma, cp, param_operands=True)
        got = g_t.cpu().numpy().reshape(npix, cp)
        _within(torch.from_numpy(np.ascontiguousarray(got[:, :ch])), (ref["g_t"][:, :ch],) + ref["bwd"], f"two_layer_tail_bwd{tag} cp={cp}")
        if has_res:
            assert np.array_equal(got[:, ch:c2], d["g_h"])    # the residual path copies g_h
        assert np.array_equal(ax.cpu().numpy().reshape(npix, ch), ref["abs_x"].astype(np.float32))
        _within(gx, (ref["gx"], 1, np.abs(ref["gx"])), f"g_h base{tag}")
        # the same launch into a buffer that holds 7.0: the padding columns are written, and written with 0
        filled = torch.full((npix, cp), 7.0, dtype=torch.float32, device=dev)
        from shallow_ntc_amd import _capi as capi
        capi.call("sntc_two_layer_tail_bwd", ops._ptr(t), ops._ptr(g_h), npix, ch, has_res, act, ops._ptr(beta), ops._ptr(gamma), cp,
                  ops._ptr(filled), None, None, ops._stream())
        assert torch.equal(filled, g_t.view(npix, cp)) and (filled[:, c2:] == 0).all()


@pytest.mark.parametrize("ch,has_res,act", K.TAIL_CASES)
def test_two_layer_hidden_and_tail_bwd(ch, has_res, act, dev):
    _tail(ch, has_res, act, K.TAIL_NPIX, dev)


@pytest.mark.parametrize("ch,has_res", [(12, 0), (48, 1)])
def test_tail_bwd_relu_and_leaky_relu_differ_at_zero(ch, has_res, dev):
    """d leaky_relu / dx is 0.2 at an exact zero of either sign (TensorFlow's LeakyReluGrad: features > 0), d relu / dx is 0."""
    d = K.tail_inputs(ch, has_res, K.TAIL_NPIX)
    zero = d["t"][:, :ch] == 0
    relu, leaky = (K.tail_reference(ch, has_res, act, K.TAIL_NPIX)["g_t"][:, :ch] for act in (3, 4))
    assert zero.sum() >= 128 and (relu[zero] == 0).all() and (leaky[zero] != 0).all()
    assert np.array_equal(leaky[zero], K.LEAKY * K.f64(d["g_h"])[zero])


@pytest.mark.parametrize("ch,has_res,act", K.TAIL_CAP_CASES)
def test_two_layer_hidden_past_the_grid_cap(ch, has_res, act, dev):
    """sntc_two_layer_hidden launches tr_grid(npix) blocks: a second trip starts at pixel TR_CAP."""
    from shallow_ntc_amd import ops
    npix = TR_CAP + 259
    assert npix > TR_CAP
    d, ref = K.tail_inputs(ch, has_res, npix), K.tail_reference(ch, has_res, act, npix)
    h = ops.two_layer_hidden(_dev(d["t"], dev).view(1, npix, 1, -1), ch, has_res, act, _dev(d["beta"], dev), _dev(d["gamma"], dev))
    _within(h, (ref["h"],) + ref["fwd"], f"two_layer_hidden[{ch},{has_res},{act},{npix}]")


@pytest.mark.parametrize("ch,has_res,act", K.TAIL_CAP_CASES)
def test_two_layer_tail_bwd_past_the_grid_cap(ch, has_res, act, dev):
    """sntc_two_layer_tail_bwd launches grid_for(npix) blocks: a second trip starts at pixel SGA_CAP."""
    npix = SGA_CAP + 259
    assert npix > SGA_CAP
    _tail(ch, has_res, act, npix, dev)


def test_two_layer_tail_bwd_refusals(dev):
    from shallow_ntc_amd import _capi as capi, ops
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
    with pytest.raises(capi.SntcError) as e:
        ops.two_layer_tail_bwd(z(1, 4, 1, 16), z(1, 4, 1, 16), 16, 0, 3, None, None, 16)
    assert e.value.code == capi.ERR_UNSUPPORTED
    with pytest.raises(capi.SntcError) as e:
        ops.two_layer_tail_bwd(z(1, 4, 1, 24), z(1, 4, 1, 12), 12, 1, 3, None, None, 23)         # cp < c2
    assert e.value.code == capi.ERR_BAD_SHAPE
    t, g, out, one = z(4, 12), z(4, 12), z(4, 12), z(4, 12)
    for ax, gx in ((one, None), (None, one)):                                                 # abs_x and g_x go together
        rc = capi.load().sntc_two_layer_tail_bwd(ops._ptr(t), ops._ptr(g), 4, 12, 0, 3, None, None, 12, ops._ptr(out), ops._ptr(ax),
                                                 ops._ptr(gx), ops._stream())
        assert rc == capi.ERR_BAD_SHAPE


# ---- 4. sntc_adam_step ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", K.ADAM_STEPS)
def test_adam_step(t, dev):
    from shallow_ntc_amd import ops
    assert K.ADAM_N > 2 * SGA_CAP
    d, ref = K.adam_inputs(), K.adam_reference(t)
    assert (d["m"] != 0).sum() >= K.ADAM_N - 64 and (d["v"] >= 0).all() and len(d["still"]) == 64
    p, g, m, v = (_dev(d[k], dev) for k in "pgmv")
    ops.adam_step(p, g, m, v, K.ADAM["lr"], t, K.ADAM["beta1"], K.ADAM["beta2"], K.ADAM["eps"], K.ADAM["grad_scale"])
    for name, got in (("m", m), ("v", v), ("p", p)):
        _within(got, ref[name], f"adam[{t}] {name}")
    still = d["still"]
    assert np.array_equal(p.cpu().numpy()[still], d["p"][still]) and torch.isfinite(p).all()     # 0 / (0 + eps): no move


# ---- 5. sntc_conv_wgrad ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,expect", K.WG_CASES, ids=K.WG_IDS)
def test_conv_wgrad_slabs_and_padding(case, expect, dev):
    from shallow_ntc_amd import _capi as capi, ops
    kind, k, s, cin, cout, n, h, w = case
    geo = K.wg_split(*case)
    nbytes = capi.load().sntc_conv_wgrad_workspace_bytes(K.WG_KINDS[kind], k, k, s, cin, cout, n, h, w)
    ksplit = nbytes // (4 * geo["M"] * geo["N"]) if nbytes else 1
    assert (geo["P"], ksplit, geo["last_slab"], geo["last_stage"]) == expect and geo["ksplit"] == ksplit
    assert n >= 2 and K.wg_stages_straddle(geo)              # 16-pixel stages run across row and image (or slab) boundaries
    c = K.wg_case(case)
    x, g = _dev(c["x"], dev), _dev(c["g"], dev)
    raw_shape = (k, k, cout, cin) if kind in ("convT", "sigup") else (k, k, cin, cout)      # what the kernel writes

    def layout(dw):                        # -> the layer's own kernel layout
        if kind != "sigup":
            return dw.cpu().numpy()
        out = torch.full((k * k, cin, cout), -1.0, dtype=torch.float32, device=dev)
        return ops.transpose_last2(dw.view(k * k, cout, cin), out).cpu().numpy().reshape(c["shape"])

    dw = torch.full(raw_shape, 7.0, dtype=torch.float32, device=dev)              # must be overwritten
    ops.conv_wgrad(kind, k, s, cin, cout, x, g, dw)
    once = layout(dw)
    q = K.worst_ratio(once, c["dw"], geo["P"] + 1, c["S"])                       # a P-term accumulation in any order
    print(f"conv_wgrad {case}: rel {K.rel(once, c['dw']):.2e}, worst / bar {q:.4f}")
    assert K.rel(once, c["dw"]) < 2e-5 and q <= 1.0
    ops.conv_wgrad(kind, k, s, cin, cout, x, g, dw, accumulate=True)               # accumulate: exactly twice
    twice = layout(dw)
    assert K.rel(twice, 2 * c["dw"]) < 2e-5 and K.worst_ratio(twice, 2 * c["dw"], geo["P"] + 2, 2 * c["S"]) <= 1.0
    dw2 = torch.empty_like(dw)
    ops.conv_wgrad(kind, k, s, cin, cout, x, g, dw2)                               # deterministic: bit-identical on a re-run
    ops.conv_wgrad(kind, k, s, cin, cout, x, g, dw)
    assert torch.equal(dw, dw2) and np.array_equal(layout(dw), once)


# ---- 6. sntc_bias_grad ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,slabs", K.BIAS_CASES)
def test_bias_grad_strips_and_slabs(shape, slabs, dev):
    from shallow_ntc_amd import _capi as capi, ops
    npix, c = shape
    assert capi.load().sntc_bias_grad_workspace_bytes(npix, c) == 4 * slabs * c and K.bias_slabs(npix, c) == slabs
    case = K.bias_case(npix, c)
    g = _dev(case["g"], dev)
    db = torch.full((c,), 7.0, dtype=torch.float32, device=dev)
    ops.bias_grad(g, db)
    once = db.cpu().numpy()
    q = K.worst_ratio(once, case["ref"], npix + 1, case["S"])
    print(f"bias_grad {shape}: rel {K.rel(once, case['ref']):.2e}, worst / bar {q:.4f}")
    assert K.rel(once, case["ref"]) < 2e-5 and q <= 1.0
    ops.bias_grad(g, db, accumulate=True)
    twice = db.cpu().numpy()
    assert K.rel(twice, 2 * case["ref"]) < 2e-5 and K.worst_ratio(twice, 2 * case["ref"], npix + 2, 2 * case["S"]) <= 1.0


# ---- 7. deep-factorized prior gradients ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,n,hw", K.PRIOR_CASES)
def test_prior_gradients(c, n, hw, dev):
    """sntc_noisy_factorized with a grad_record, then sntc_prior_param_grad, as Trainer._loss_and_grads calls them."""
    from shallow_ntc_amd import _capi as capi, ops
    mats, biases, factors = K.prior_params(c)
    ref = K.prior_case(c, n, hw)
    prior = ops.DeepFactorizedPrior(list(mats), list(biases), list(factors))
    flat = lambda grp: _dev(np.concatenate([a.ravel() for a in grp]), dev)
    pm, pf = flat(mats), flat(factors)
    z = _dev(ref["z"], dev)
    rec = torch.full((capi.load().sntc_prior_record_floats(prior._h),), 7.0, dtype=torch.float32, device=dev)     # must be overwritten

    def run(weight):
        dz = torch.empty_like(z)
        bits = torch.empty((n,), dtype=torch.float64, device=dev)
        capi.call("sntc_noisy_factorized", prior._h, ops._ptr(z), n, hw, ops._ptr(dz), ops._ptr(rec), ops._ptr(bits), ops._stream())
        return bits.cpu().numpy(), dz.cpu().numpy(), grads(weight)

    def grads(weight):
        gm, gb, gf = torch.empty_like(pm), torch.empty((sum(a.size for a in biases),), device=dev), torch.empty_like(pf)
        capi.call("sntc_prior_param_grad", prior._h, ops._ptr(pm), ops._ptr(pf), ops._ptr(rec), weight, ops._ptr(gm), ops._ptr(gb),
                  ops._ptr(gf), ops._stream())
        return [t.cpu().numpy() for t in (gm, gb, gf)]

    bits, dz, full = run(1.0)
    quarter = grads(0.25)                                    # the same record: exactly a quarter
    worst = dict(bits=K.rel(bits, ref["bits"]), dz=K.rel(dz, ref["dz"]), gm=K.rel(full[0], ref["gm"]), gb=K.rel(full[1], ref["gb"]),
                 gf=K.rel(full[2], ref["gf"]))
    print(f"prior [{c},{n},{hw}]: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) < 2e-5, worst
    for a, b in zip(quarter, full):
        assert np.array_equal(a, np.float32(0.25) * b)
    bits2, dz2, again = run(1.0)                             # the record lands by float atomics: 1e-6 between runs
    assert np.array_equal(dz2, dz)
    assert K.rel(bits2, bits) < 1e-12
    for a, b in zip(again, full):
        assert K.rel(a, b) < 1e-6
