"""Rate-distortion optimised quantisation (-m gpu; DESIGN.md 4.7, "RDOQ"): the kernels of csrc/rdoq.hip against their float32
NumPy restatement (``np_rdoq``, integer equality), their identities, ``compress(x, rdoq=...)`` / ``coded_cost(x, rdoq=...)``,
``Model.latent_gains`` against the float64 oracle synthesis, and the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_hip_itinf_bitstream import big_table_set, fact_model, hyper_model, image_words, images  # noqa: F401
from test_hip_quant_step import case_of, dev_case, dv, offset_view, sse_of
from test_rans_cost_host import np_cost, np_symbols, ref_cost_table

pytestmark = pytest.mark.gpu

KERNEL_CASES = [(1028, 4, 4), (4100, 4, 8), (960, 320, 640), (70080, 320, 320)]
KS = [5, -32]                  # images 1 and 0 of the step cases (test_hip_quant_step.STEPS): their planted ties are at these steps
UNIT = 65536.0


def np_rdoq(y, mu, ids, k, weight, enable, flags, tabs, q):
    """The rule of csrc/rdoq_rules.h in float32 NumPy, every operation one rounding.  y / mu / ids [n, hw, c]; ``k`` the ladder
    index, [n, 1, 1] (per image) or [n, hw, 1] (a map; clamped into [-32, 32] as the kernels clamp a map's byte); weight [c];
    enable [n]; q = ref_cost_table(tabs).  The conversion to int is the device's: NaN -> 0, saturating.
    -> (symbols int32, table ids int16, changed int64 [n], s0 int32)."""
    from shallow_ntc_amd import entropy_coding as ec
    f32 = np.float32
    k = np.clip(np.asarray(k, np.int64), -32, 32)
    inv = np.array([ec.step_size(-j) for j in range(-32, 33)], f32)[k + 32]
    w = np.asarray(weight, f32).reshape(1, 1, -1)
    with np.errstate(invalid="ignore", over="ignore"):
        d = y.astype(f32) - mu.astype(f32)
        u = (d * inv).astype(f32)
        r = np.rint(u.astype(np.float64))
        s0 = np.where(np.isnan(r), 0.0, np.clip(r, -2.0 ** 31, 2.0 ** 31 - 1)).astype(np.int64)
        t = np.clip(ids.astype(np.int64) - k, 0, 63)

        def cost(s):
            e = u - s.astype(f32)                                   # float32 - float32: one rounding
            price = np.asarray(q)[np_symbols(s, t, tabs)[0]].astype(f32)   # below 2^22: exact
            return w * (e * e) + price                              # float32 throughout: a rounding per operation

        live = (np.asarray(enable).reshape(-1, 1, 1) != 0) & (s0 != 0)
        best, jb = s0.copy(), cost(s0)
        a = s0 - np.sign(s0)
        ja = cost(a)
        take = live & (ja < jb)
        best, jb = np.where(take, a, best), np.where(take, ja, jb)
        if flags & 1:
            take = live & (a != 0) & (cost(np.zeros_like(s0)) < jb)
            best = np.where(take, 0, best)
    assert d.dtype == f32 and u.dtype == f32 and jb.dtype == f32
    changed = (best != s0).reshape(s0.shape[0], -1).sum(axis=1)
    return best.astype(np.int32), t.astype(np.int16), changed.astype(np.int64), s0.astype(np.int32)


def case_weights(c, seed=0):
    """Per-channel weights in cost_q units around one bit per squared symbol unit, where both outcomes happen; channel 0 weighs
    nothing (with a non-finite u its J is NaN) and one channel weighs so much that nothing changes."""
    w = (np.random.default_rng(seed + c).uniform(0.05, 4.0, c) * UNIT).astype(np.float32)
    w[0], w[c - 1] = 0.0, 1e30
    return w


_rdoq_cases = {}


def rdoq_case(E, c, stride):
    """Two images of the step case of this shape (its images 1 and 0, at KS) with the hard elements planted into both, and a
    map over the whole ladder with stray bytes.  Built once per shape."""
    from shallow_ntc_amd import entropy_coding as ec
    key = (E, c, stride)
    if key in _rdoq_cases:
        return _rdoq_cases[key]
    cs = case_of(E, c, stride)
    y, rows, ids = (np.ascontiguousarray(cs[name][[1, 0]]).copy() for name in ("y", "rows", "ids"))
    hw = cs["hw"]
    fy, fm = y.reshape(2, -1), rows[..., :c]
    rng = np.random.default_rng(E + c)
    for b, k in enumerate(KS):
        step = np.float32(ec.step_size(k))
        # in units of the step: s0 = +-1 on both sides of it, exact zeros, symbols past every table, |u| > 32767
        plant = [1.0, -1.0, 0.6, -0.6, 1.4, -1.4, 0.0, 0.0, 300.0, -300.0, 40000.0, -50000.0, 2.4, -2.4, 3.5001, -7.49]
        at = 16 + np.arange(len(plant))
        flat_mu = np.ascontiguousarray(fm[b]).reshape(-1)
        fy[b, at] = flat_mu[at] + np.array(plant, np.float32) * step
        fy[b, 40:43] = [np.nan, np.inf, -np.inf]
    kmap = rng.integers(-32, 33, size=(2, hw)).astype(np.int8)
    kmap[:, 0] = [100, -100]                                      # stray bytes: clamped to the ladder's ends
    if hw > 5:
        kmap[:, 5] = [-128, 127]
    out = dict(E=E, c=c, hw=hw, stride=stride, y=y, rows=rows, mu=rows[..., :c], ids=ids, kmap=kmap, w=case_weights(c))
    _rdoq_cases[key] = out
    return out


@pytest.fixture(scope="module")
def normal(dev):
    from shallow_ntc_amd import entropy_coding as ec
    tabs = ec.normal_tables()
    return tabs, ec.DeviceTables(tabs, dev), ref_cost_table(tabs)


def on_device(cs, dev):
    y, hyper, ids = dev_case(cs, dev)
    return y, hyper, ids, dv(cs["w"], dev), dv(cs["kmap"], dev).view(2, cs["hw"], 1)


def i32(vals, dev):
    return torch.tensor(vals, dtype=torch.int32, device=dev)


# ------------------------------------------------------------------ kernels ------------------------------------------------
@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("E,c,stride", KERNEL_CASES, ids=[f"E{E}-c{c}-stride{s}" for E, c, s in KERNEL_CASES])
def test_rdoq_symbols_are_the_float32_rule(E, c, stride, flags, dev, normal):
    from shallow_ntc_amd import entropy_coding as ec
    from shallow_ntc_amd import ops
    tabs, dt, q = normal
    cs = rdoq_case(E, c, stride)
    y, hyper, ids, w, kmap = on_device(cs, dev)
    _, inv, sh = ec.step_tensors(KS, dev)
    lut = ec.step_lut(dev)
    seen = set()
    for enable in ([1, 0], [0, 1]):
        en = i32(enable, dev)
        for mapped in (False, True):
            k = cs["kmap"].astype(np.int64)[..., None] if mapped else np.array(KS, np.int64).reshape(2, 1, 1)
            want_sym, want_tid, want_changed, s0 = np_rdoq(cs["y"], cs["mu"], cs["ids"], k, cs["w"], enable, flags, tabs, q)
            if mapped:
                sym, tid, changed = ops.rdoq_map_symbols(y, hyper, ids, kmap, lut, w, en, flags, dt)
            else:
                sym, tid, changed = ops.rdoq_symbols(y, hyper, ids, inv, sh, w, en, flags, dt)
            shape = tuple(sym.shape)
            assert torch.equal(sym, dv(want_sym, dev).view(shape)), (enable, mapped)
            assert torch.equal(tid, dv(want_tid, dev).view(shape)), (enable, mapped)
            assert changed.dtype == torch.int32 and torch.equal(changed.to(torch.int64), dv(want_changed, dev)), (enable, mapped)
            b = enable.index(1)
            assert want_changed[b] > 0 and want_changed[1 - b] == 0
            moved = want_sym[b] != s0[b]
            seen |= {"towards zero"} if (moved & (want_sym[b] != 0)).any() else set()
            seen |= {"zero from afar"} if (moved & (want_sym[b] == 0) & (np.abs(s0[b]) > 1)).any() else set()
            if not mapped:                                   # the planted elements are what they claim, at each image's own step
                u = ((cs["y"][b] - cs["mu"][b]).astype(np.float32) * np.float32(ec.step_size(-KS[b]))).astype(np.float32).reshape(-1)
                flat = s0[b].reshape(-1)
                with np.errstate(invalid="ignore"):
                    assert (u - np.floor(u) == 0.5).any() and (flat == 1).any() and (flat == -1).any() and (u == 0).any()
                    assert (np.abs(u) > 32767).any() and np.isnan(u).any() and np.isposinf(u).any() and np.isneginf(u).any()
                assert (np_symbols(flat, want_tid[b].reshape(-1), tabs)[1]).any()          # escapes
                assert flat[40] == 0 and flat[41] == 2 ** 31 - 1 and flat[42] == -2 ** 31    # NaN, +inf, -inf
    assert "towards zero" in seen and (not flags or "zero from afar" in seen)


def test_rdoq_with_tables_beyond_the_lds_limit(dev):
    """Descriptors and prices read from global memory (84 tables; the ladder is their first 64): the same integers."""
    from shallow_ntc_amd import entropy_coding as ec
    from shallow_ntc_amd import ops
    big = big_table_set()
    db, q = ec.DeviceTables(big, dev), ref_cost_table(big)
    cs = rdoq_case(4100, 4, 8)
    y, hyper, ids, w, kmap = on_device(cs, dev)
    _, inv, sh = ec.step_tensors(KS, dev)
    en = i32([1, 1], dev)
    want = np_rdoq(cs["y"], cs["mu"], cs["ids"], np.array(KS).reshape(2, 1, 1), cs["w"], [1, 1], 1, big, q)
    sym, tid, changed = ops.rdoq_symbols(y, hyper, ids, inv, sh, w, en, 1, db)
    assert torch.equal(sym, dv(want[0], dev).view(sym.shape)) and torch.equal(tid, dv(want[1], dev).view(tid.shape))
    assert changed.tolist() == want[2].tolist() and min(changed.tolist()) > 0
    want = np_rdoq(cs["y"], cs["mu"], cs["ids"], cs["kmap"].astype(np.int64)[..., None], cs["w"], [1, 1], 1, big, q)
    sym, tid, changed = ops.rdoq_map_symbols(y, hyper, ids, kmap, ec.step_lut(dev), w, en, 1, db)
    assert torch.equal(sym, dv(want[0], dev).view(sym.shape)) and torch.equal(tid, dv(want[1], dev).view(tid.shape))
    assert changed.tolist() == want[2].tolist()


def test_rdoq_identities(dev, normal):
    from shallow_ntc_amd import entropy_coding as ec
    from shallow_ntc_amd import ops
    tabs, dt, q = normal
    lut = ec.step_lut(dev)
    for key in ((4100, 4, 8), (960, 320, 640)):
        cs = rdoq_case(*key)
        y, hyper, ids, w, kmap = on_device(cs, dev)
        _, inv, sh = ec.step_tensors(KS, dev)
        off, both = i32([0, 0], dev), i32([1, 1], dev)
        plain, plain_map = ops.step_symbols(y, hyper, ids, inv, sh), ops.step_map_symbols(y, hyper, ids, kmap, lut)
        # every enable 0: the step kernels, bit for bit
        for flags in (0, 1):
            got = ops.rdoq_symbols(y, hyper, ids, inv, sh, w, off, flags, dt)
            assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1]) and got[2].tolist() == [0, 0]
            got = ops.rdoq_map_symbols(y, hyper, ids, kmap, lut, w, off, flags, dt)
            assert torch.equal(got[0], plain_map[0]) and torch.equal(got[1], plain_map[1]) and got[2].tolist() == [0, 0]
        assert ops.rdoq_symbols(y, hyper, ids, inv, sh, w, off, 1, dt, want_changed=False)[2] is None
        # a constant map: the per-image kernel at that index
        const = dv(np.repeat(np.array(KS, np.int8)[:, None], cs["hw"], axis=1), dev).view(2, cs["hw"], 1)
        for flags in (0, 1):
            a = ops.rdoq_symbols(y, hyper, ids, inv, sh, w, both, flags, dt)
            b = ops.rdoq_map_symbols(y, hyper, ids, const, lut, w, both, flags, dt)
            assert all(torch.equal(p, r) for p, r in zip(a, b))
            # bits never rise, and fall wherever a symbol changed -- as integers
            for (sym, tid, changed), (psym, ptid) in ((a, plain), (ops.rdoq_map_symbols(y, hyper, ids, kmap, lut, w, both, flags, dt), plain_map)):
                assert torch.equal(tid, ptid)
                cost, cost0 = ec.rans_cost(sym, tid, dt).tolist(), ec.rans_cost(psym, ptid, dt).tolist()
                for i in range(2):
                    assert changed[i].item() > 0 and cost[i] < cost0[i], (key, flags, i, cost, cost0)
                assert cost == np_cost(sym.cpu().numpy().reshape(2, -1), tid.cpu().numpy().reshape(2, -1), tabs, q).tolist()
        # weight 0: the first of the cheapest candidates, from the integer prices alone (finite u; elsewhere J is NaN: s0)
        zero_w = torch.zeros_like(w)
        sym = ops.rdoq_symbols(y, hyper, ids, inv, sh, zero_w, both, 1, dt)[0].cpu().numpy().reshape(cs["y"].shape).astype(np.int64)
        s0, tid = plain[0].cpu().numpy().reshape(cs["y"].shape).astype(np.int64), plain[1].cpu().numpy().reshape(cs["y"].shape)
        price = lambda s: np.asarray(q)[np_symbols(s, tid, tabs)[0]].astype(np.int64)
        a = s0 - np.sign(s0)
        want, best = s0.copy(), price(s0)
        take = (s0 != 0) & (price(a) < best)
        want, best = np.where(take, a, want), np.where(take, price(a), best)
        want = np.where((s0 != 0) & (a != 0) & (price(np.zeros_like(s0)) < best), 0, want)
        finite = np.isfinite(cs["y"])
        assert (sym[finite] == want[finite]).all() and (sym[~finite] == s0[~finite]).all() and (want != s0).any()


def test_kernel_refusals(dev, normal):
    from shallow_ntc_amd import _capi as capi
    from shallow_ntc_amd import entropy_coding as ec
    from shallow_ntc_amd import ops
    _, dt, _ = normal
    lib = capi.load()
    n, hw, c = 2, 5, 8
    y = torch.zeros((n, hw, 1, c), dtype=torch.float32, device=dev)
    ids = torch.zeros((n, hw, 1, c), dtype=torch.int16, device=dev)
    _, inv, sh = ec.step_tensors([1, -1], dev)
    sym = torch.zeros((n, hw, 1, c), dtype=torch.int32, device=dev)
    kmap, lut = torch.zeros((n, hw, 1), dtype=torch.int8, device=dev), ec.step_lut(dev)
    w, en, ch = torch.ones(c, device=dev), i32([1, 1], dev), i32([7, 7], dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = ops._stream()

    def per_image(yp=p(y), mp=p(y), ip=p(ids), vp=p(inv), sp=p(sh), wp=p(w), ep=p(en), mt=p(dt.meta), cq=p(dt.cost_q), op=p(sym), tp=p(ids),
                  cp=p(ch), cc=c, stride=c, nn=n, nt=dt.ntables):
        return lib.sntc_rdoq_symbols(yp, mp, nn, hw, cc, stride, ip, vp, sp, wp, ep, 1, mt, nt, dt.total, cq, op, tp, cp, stream)

    def mapped(yp=p(y), mp=p(y), ip=p(ids), kp=p(kmap), lp=p(lut), wp=p(w), ep=p(en), mt=p(dt.meta), cq=p(dt.cost_q), op=p(sym), tp=p(ids),
               cp=p(ch), cc=c, stride=c, nn=n, nt=dt.ntables):
        return lib.sntc_rdoq_map_symbols(yp, mp, nn, hw, cc, stride, ip, kp, lp, wp, ep, 1, mt, nt, dt.total, cq, op, tp, cp, stream)

    null, bad = C.c_void_p(0), capi.ERR_BAD_SHAPE
    assert per_image() == capi.OK and mapped() == capi.OK and ch.tolist() == [0, 0]      # zeroed by the launch
    assert per_image(cp=null) == capi.OK and mapped(cp=null) == capi.OK                 # changed is optional
    for call, names in ((per_image, ("yp", "mp", "ip", "vp", "sp", "wp", "ep", "mt", "cq", "op", "tp")),
                        (mapped, ("yp", "mp", "ip", "kp", "lp", "wp", "ep", "mt", "cq", "op", "tp"))):
        for name in names:
            assert call(**{name: null}) == bad, name
        assert call(cc=6, stride=6) == bad and call(cc=2, stride=4) == bad and call(stride=4) == bad and call(stride=10) == bad
        assert call(nn=0) == bad and call(nn=65536) == bad and call(nt=63) == bad
        assert call(yp=C.c_void_p(y.data_ptr() + 4)) == bad and call(op=C.c_void_p(sym.data_ptr() + 8)) == bad
        assert call(ip=C.c_void_p(ids.data_ptr() + 2)) == bad and call(wp=C.c_void_p(w.data_ptr() + 4)) == bad
    torch.cuda.synchronize()
    assert "sntc_rdoq" in capi.last_error()
    # the wrappers: an offset view is refused by the library (no element-wise path), wrong companions by the wrapper
    y2 = offset_view(y, 1, dev)
    assert y2.data_ptr() % 16 == 4
    with pytest.raises(capi.SntcError) as e:
        ops.rdoq_symbols(y2, y, ids, inv, sh, w, en, 1, dt)
    assert e.value.code == bad
    with pytest.raises(capi.SntcError):
        ops.rdoq_map_symbols(y2, y, ids, kmap, lut, w, en, 1, dt)
    for kw in (dict(weight=w[:4].contiguous()), dict(weight=w.double()), dict(enable=en.long()), dict(enable=i32([1], dev))):
        args = dict(weight=w, enable=en)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.rdoq_symbols(y, y, ids, inv, sh, args["weight"], args["enable"], 1, dt)
        with pytest.raises(ValueError):
            ops.rdoq_map_symbols(y, y, ids, kmap, lut, args["weight"], args["enable"], 1, dt)


# ------------------------------------------------------------------ model --------------------------------------------------
def two_level(model, n, h, w):
    lh, lw = model.step_offsets_shape(h, w)
    off = np.zeros((n, lh, lw), np.int8)
    off[:, :, lw // 2:] = 6
    return off


MODEL_CASES = [(2, 64, 64), (1, 200, 120)]


def cost_kwargs(model, rep, kw):
    """How ``compress(x, rdoq=...)`` judges: the weighted J on a map, else lambda_i = lambda / step_i^2 per image."""
    if kw.get("step_offsets") is not None:
        return dict(kw, weighted=True)
    return dict(kw, lam=[r["lam"] for r in rep])


@pytest.mark.parametrize("variant", ["unit", "steps", "offsets"])
@pytest.mark.parametrize("n,h,w", MODEL_CASES, ids=["2x64x64", "1x200x120"])
def test_compress_with_rdoq(n, h, w, variant, dev, hyper_model):
    from shallow_ntc_amd import entropy_coding as ec
    from shallow_ntc_amd.mshyper.models import step_lambdas
    model = hyper_model
    x = images(n, h, w, dev)
    kw = dict(unit={}, steps=dict(step=[-4, 2][:n]), offsets=dict(step=[-4, 2][:n], step_offsets=two_level(model, n, h, w)))[variant]
    for cfg in (True, dict(strength=0.25, zero=False)):
        blob = model.compress(x, rdoq=cfg, **kw)
        rep = [dict(r) for r in model.last_compress_report]
        assert blob[:4] == b"SNTC" and blob[4] == dict(unit=3, steps=5, offsets=7)[variant]
        px = model.decompress(blob)
        sse = sse_of(px, x).tolist()
        ck = cost_kwargs(model, rep, kw)
        plain, cand = model.coded_cost(x, **ck), model.coded_cost(x, rdoq=cfg, **ck)
        lam = float(model._scheduled_rd_lambda)
        for i, r in enumerate(rep):
            print(f"\n{variant} {n}x{h}x{w} image {i} {cfg}: changed {r['changed']}, bits {r['bits_plain']:.1f} -> {r['bits_rdoq']:.1f}, "
                  f"sse {r['sse_plain']:.0f} -> {r['sse_rdoq']:.0f}, J {r['J_plain']:.6f} -> {r['J_rdoq']:.6f}, used {r['rdoq_used']}")
            assert (r["bits_plain"], r["sse_plain"], r["J_plain"]) == (plain["bits"][i], plain["sse"][i], plain["J"][i])
            assert (r["bits_rdoq"], r["sse_rdoq"], r["J_rdoq"], r["changed"]) == (cand["bits"][i], cand["sse"][i], cand["J"][i], cand["changed"][i])
            assert r["rdoq_used"] == (r["J_rdoq"] < r["J_plain"]) and r["J_chosen"] == min(r["J_plain"], r["J_rdoq"])
            assert sse[i] == (r["sse_rdoq"] if r["rdoq_used"] else r["sse_plain"]) == r["sse_chosen"]
            assert r["bits_rdoq"] <= r["bits_plain"] and (r["changed"] == 0 or r["bits_rdoq"] < r["bits_plain"])
            assert r["quant_step"] == (kw["step"][i] if "step" in kw else 0)
            if variant != "offsets":
                assert r["lam"] == step_lambdas(lam, [r["quant_step"]])[0]
        if not any(r["rdoq_used"] for r in rep):
            assert blob == model.compress(x, **kw)
    assert set(rep[0]) >= {"rdoq_used", "changed", "bits_plain", "bits_rdoq", "sse_plain", "sse_rdoq", "J_plain", "J_rdoq", "lam", "quant_step"}


def test_rdoq_gains_and_strength(dev, hyper_model):
    model = hyper_model
    c = model._bottleneck_size
    n, h, w = 2, 64, 64
    x = images(n, h, w, dev)
    # gains so large that no symbol can pay for a move: nothing changes, the file is the plain one
    for kw in ({}, dict(step=[-4, 2]), dict(step=[-4, 2], step_offsets=two_level(model, n, h, w))):
        blob = model.compress(x, rdoq=dict(gains=np.full(c, 1e30)), **kw)
        assert [r["changed"] for r in model.last_compress_report] == [0, 0] and not any(r["rdoq_used"] for r in model.last_compress_report)
        assert blob == model.compress(x, **kw)
    # a weak weight at a fine step: symbols move on every image, and the bits fall
    model.compress(x, step=-4, rdoq=dict(strength=1e-3))
    for r in model.last_compress_report:
        assert r["changed"] > 0 and r["bits_rdoq"] < r["bits_plain"]
    cost = model.coded_cost(x, step=-4, rdoq=dict(strength=1e-3))
    assert cost["changed"].tolist() == [r["changed"] for r in model.last_compress_report] and cost["changed"].dtype == np.int64
    # max_error on top: the layered file of the rdoq file, within the bound
    blob = model.compress(x, step=2, rdoq=dict(strength=1e-3), max_error=2)
    assert blob[4] == 8 and all("rdoq_used" in r and r["max_error"] == 2 for r in model.last_compress_report)
    want = np.rint((x.cpu().numpy().astype(np.float64) + 0.5) * 255)
    assert np.abs(model.decompress(blob).cpu().numpy().astype(np.int64) - want).max() <= 2


def test_rdoq_enable_list_through_compress_latents(dev, hyper_model):
    from shallow_ntc_amd import entropy_coding as ec
    model = hyper_model
    codec = model._get_codec()
    n, h, w = 2, 64, 64
    x = images(n, h, w, dev)
    lat = model.infer_latent_rvs(x)
    z, y = lat.uq[0].loc.contiguous(), lat.uq[1].loc.contiguous()
    weight = ec.rdoq_weights(float(model._scheduled_rd_lambda), model.latent_gains(), 1e-3)
    for kw in (dict(step=-4), dict(step=[-6, -4])):             # fine steps: these small images have symbols to move on both
        tool = codec.rdoq(weight, n)
        plain = codec.compress_latents(z, y, (h, w), **kw)
        both = codec.compress_latents(z, y, (h, w), rdoq=tool, **kw)
        assert tool.changed.tolist()[0] > 0 and tool.changed.tolist()[1] > 0
        first = codec.compress_latents(z, y, (h, w), rdoq=tool, rdoq_enable=[1, 0], **kw)
        assert tool.changed.tolist()[0] > 0 and tool.changed.tolist()[1] == 0
        assert image_words(model, first, 1) == image_words(model, plain, 1) and image_words(model, first, 0) == image_words(model, both, 0)
        assert image_words(model, first, 0) != image_words(model, plain, 0)
        assert codec.compress_latents(z, y, (h, w), rdoq=tool, rdoq_enable=[0, 0], **kw) == plain
        assert torch.equal(model.decompress(first)[1], model.decompress(plain)[1])
    with pytest.raises(ValueError):
        codec.compress_latents(z, y, (h, w), rdoq_enable=[1, 0])
    with pytest.raises(ValueError):
        codec.compress_latents(z, y, (h, w), rdoq=codec.rdoq(weight, n), rdoq_enable=[1, 2])
    with pytest.raises(ValueError):
        codec.rdoq(weight[:8], n)


# ------------------------------------------------------------------ gains --------------------------------------------------
GAIN_SYNTHS = [dict(cls="JPEGLikeSynthesis", kernel_size=18, strides=16),
               dict(cls="TwoLayerResSynthesis", channels=(12, 3), strides=(8, 2), kernel_sizes=(13, 5), activation_type="igdn", res_type="conv")]


@pytest.mark.parametrize("synth", GAIN_SYNTHS, ids=["jpeg-like", "two-layer-res"])
def test_latent_gains_against_the_float64_synthesis(synth, dev):
    """g_c against the float64 oracle synthesis of the same weights on the same impulses.  The bar: test_hip_model's
    test_transform_parity holds this synthesis' output to 5e-5 of its largest value; g sums squares of output differences, and
    the relative error of a square is twice that of the value: 1e-4 of the largest gain."""
    from oracle import transforms_np as T
    from shallow_ntc_amd.mshyper.models import Model
    from test_hip_model import randomize, rel_err
    tc = dict(analysis=dict(cls="ElicAnalysis", channels=(32, 32, 32, 64)), synthesis=synth)
    model = Model(rd_lambda=0.02, transform_config=tc, device=dev)
    c = model._bottleneck_size
    w = dict(model.get_weights())
    sw = randomize({k[len("synthesis/"):]: v for k, v in w.items() if k.startswith("synthesis/")}, np.random.default_rng(5))
    w.update({f"synthesis/{k}": v for k, v in sw.items()})
    model.set_weights(w)
    got = model.latent_gains()
    assert got.dtype == np.float64 and got.shape == (c,) and (got > 0).all()
    assert model.latent_gains() is not got and np.array_equal(model.latent_gains(), got)          # cached; the caller's copy is its own
    okw = {k: v for k, v in synth.items() if k != "cls"}
    ref_t = T.build(synth["cls"], cin=c, **okw)
    y = np.zeros((c + 1, 9, 9, c), np.float32)
    y[np.arange(c), 4, 4, np.arange(c)] = 1.0
    out = np.asarray(ref_t(sw, y), np.float64)
    d = 255.0 * (out[:c] - out[c:])
    b = out.shape[1] // 9
    ring = d.copy()
    ring[:, b:-b, b:-b] = 0.0
    assert out.shape[1] == out.shape[2] == 9 * b and not ring.any()                              # the zero outer ring, in float64 too
    want = (d * d).reshape(c, -1).sum(axis=1)
    print(f"\n{synth['cls']}: gains {want.min():.4g} .. {want.max():.4g}, relative error {rel_err(got, want):.3g}")
    assert rel_err(got, want) < 2 * 5e-5
    model.set_weights(w)
    assert model._latent_gains is None                                                           # new weights: computed again


# ------------------------------------------------------------------ refusals -----------------------------------------------
def test_refusals(dev, hyper_model, fact_model, monkeypatch):
    from shallow_ntc_amd.mshyper.models import Model
    from test_hip_sga import TC
    model = hyper_model
    c = model._bottleneck_size
    x = images(2, 64, 64, dev)
    launches = []
    for m in (model, fact_model):
        analysis = m.infer_latent_rvs
        monkeypatch.setattr(m, "infer_latent_rvs", lambda *a, _f=analysis, **k: launches.append(1) or _f(*a, **k))
    monkeypatch.setattr(model, "latent_gains", lambda: launches.append(1))
    for call in (model.compress, model.coded_cost):
        for bad in (dict(strength=0.0), dict(strength=-1.0), dict(strength=float("nan")), dict(strength=float("inf")), dict(strength="x"),
                    dict(gains=np.ones(c - 1)), dict(gains=np.ones((c, 1))), dict(gains=-np.ones(c)), dict(gains=np.full(c, np.nan)),
                    dict(power=2), 1, "yes"):
            with pytest.raises(ValueError):
                call(x, rdoq=bad)
        with pytest.raises(ValueError):
            call(x, rdoq=True, step=33)
    for kw in (dict(itinf=dict(steps=2)), dict(target_bpp=0.3), dict(target_psnr=33.0)):
        with pytest.raises(ValueError, match="rdoq excludes"):
            model.compress(x, rdoq=True, **kw)
    for call in (fact_model.compress, fact_model.coded_cost):
        with pytest.raises(NotImplementedError, match="factorized"):
            call(x, rdoq=True)
    for over in (dict(precision="bf16x3"), dict(distortion="ms_ssim")):
        other = Model(device=dev, rd_lambda=0.02, transform_config=TC, **over)
        monkeypatch.setattr(other, "infer_latent_rvs", lambda *a, **k: launches.append(1))
        for call in (other.compress, other.coded_cost):
            with pytest.raises(NotImplementedError, match=list(over.values())[0]):
                call(x, rdoq=True)
    assert not launches                                         # every refusal came before the analysis ran
