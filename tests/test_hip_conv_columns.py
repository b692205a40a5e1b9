"""Column-limited launches of a gather-GEMM plan (sntc_conv_forward_columns, ops.ConvPlan.columns) and the decoder's mean-only
hyper-synthesis built on them: the first ``ncols`` output channels of a layer, from the same plan and packed weights, are the
SAME BITS as the leading slice of the whole layer -- under every tile variant and schedule -- and everything the launch does not
cover is refused before anything runs."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import ops_np as O

pytestmark = pytest.mark.gpu

TOL = 2e-5      # tests/test_hip_ops.py, conv family: float32 accumulation against float64 (max error / max magnitude)


def dev_t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


def rel_err(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


_LAYERS = {}


def layer(cin, cout, n, h, w, dev):
    """One transposed 3x3 / 1 layer, its input and its whole-layer output (computed once per shape, shared, never modified)."""
    from shallow_ntc_amd import ops
    key = (cin, cout, n, h, w)
    if key not in _LAYERS:
        rng = np.random.default_rng(1000 * cin + 10 * n + h)
        wk = (rng.standard_normal((3, 3, cout, cin)) / np.sqrt(9 * cin / 4)).astype(np.float32)
        b = rng.standard_normal(cout).astype(np.float32)
        x = rng.standard_normal((n, h, w, cin)).astype(np.float32)
        plan = ops.ConvPlan("convT", dev_t(wk, dev), dev_t(b, dev), 1)
        xd = dev_t(x, dev)
        _LAYERS[key] = dict(plan=plan, x=xd, full=plan(xd), host=(x, wk, b))
    return _LAYERS[key]


def every_schedule(plan, view, x, want):
    """``view(x)`` under every (variant, stream_k) candidate of the limited launch and under the two forced stream-K orders."""
    n, h, w = (int(v) for v in x.shape[:3])
    cands = view.candidates(n, h, w)
    assert cands
    try:
        for v, sk in cands:
            view.set_choice(n, h, w, v, sk)
            assert view.launch_info(n, h, w)[0] == v
            got = view(x)
            assert got.shape == want.shape and got.is_contiguous()
            assert torch.equal(got, want), (v, sk)
    finally:
        view.drop_choice(n, h, w)
    try:
        for colm in (False, True):
            plan.set_stream_k(True, force=True, colm=colm)
            assert torch.equal(view(x), want), ("forced stream-K", colm)
    finally:
        plan.set_stream_k(True)
    return cands


CASES = ([(96, 192, 2, 12, 20, nc) for nc in (64, 96, 100, 128, 192)] +        # M = 480: no multiple of 128 or 64
         [(96, 192, 1, 5, 7, nc) for nc in (64, 96, 100, 128, 192)] +
         [(480, 640, 1, 8, 12, nc) for nc in (320, 640)])


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_limited_launch_is_the_leading_slice_bit_for_bit(case, dev):
    cin, cout, n, h, w, ncols = case
    L = layer(cin, cout, n, h, w, dev)
    plan = L["plan"]
    assert plan.columns_supported(ncols)
    view = plan.columns(ncols)
    assert view.cout == ncols and view.flops(n, h, w) * cout == plan.flops(n, h, w) * ncols
    want = L["full"][..., :ncols].contiguous()
    every_schedule(plan, view, L["x"], want)
    assert torch.equal(view(L["x"]), want)                       # the cost model's own pick
    assert torch.equal(plan(L["x"]), L["full"])                  # the whole layer is what it was


def test_limited_launch_under_real_stream_k(dev):
    """Large enough (32768 rows: 256 tiles of 128 rows and more) that the stream-K candidates exist and the hand-off
    continuation really writes compact rows -- the shapes above are too small for any worker to share a tile."""
    L = layer(96, 192, 8, 64, 64, dev)
    view = L["plan"].columns(96)
    cands = every_schedule(L["plan"], view, L["x"], L["full"][..., :96].contiguous())
    assert any(sk for _, sk in cands), cands


def test_refusals_come_before_any_launch(dev):
    from shallow_ntc_amd import _capi as capi
    from shallow_ntc_amd import ops
    L = layer(96, 192, 1, 5, 7, dev)
    plan, x = L["plan"], L["x"]
    lib = capi.load()
    y = torch.full((1, 5, 7, 196), 7.0, device=dev)
    ws = torch.empty((1 << 20,), device=dev)
    refused = (capi.ERR_UNSUPPORTED, capi.ERR_BAD_SHAPE)

    def launch(p, ncols):
        return lib.sntc_conv_forward_columns(p._h, x.data_ptr(), 1, 5, 7, y.data_ptr(), None, None, ws.data_ptr(), ws.numel() * 4,
                                             None, ncols)

    for ncols in (0, 98, plan.cout + 4):
        assert not plan.columns_supported(ncols)
        assert launch(plan, ncols) in refused
        with pytest.raises(capi.SntcError) as e:
            plan.columns(ncols)
        assert e.value.code in refused
    rng = np.random.default_rng(3)
    up2 = ops.ConvPlan("convT", dev_t(rng.standard_normal((5, 5, 64, 96)) * 0.05, dev), None, 2)       # several phase groups
    bf3 = ops.ConvPlan("convT", dev_t(rng.standard_normal((3, 3, 192, 96)) * 0.05, dev), None, 1, bf16x3=True)
    for p in (up2, bf3):
        assert not p.columns_supported(32)
        assert launch(p, 32) in refused
        with pytest.raises(capi.SntcError) as e:
            p.columns(32)
        assert e.value.code in refused
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())           # nothing was written


def test_limited_launch_against_float64(dev):
    L = layer(96, 192, 2, 12, 20, dev)
    x, wk, b = L["host"]
    ref = O.conv2d_transpose(x, wk[:, :, :96], b[:96], 1)
    got = L["plan"].columns(96)(L["x"]).cpu().numpy()
    assert got.shape == ref.shape
    err = rel_err(got, ref)
    print(f"columns(96) against float64: {err:.3e} (bound {TOL})")
    assert err < TOL


@pytest.fixture(scope="module")
def model(dev):
    from shallow_ntc_amd.mshyper import configs
    from shallow_ntc_amd.mshyper.models import Model
    m = Model(device=dev, **configs.two_layer_syn(rd_lambda=0.005))
    w = m.get_weights()
    b = w["hyper_synthesis/layer_2/bias"].copy()
    b[320:] = np.random.default_rng(4321).uniform(-2.0, 2.5, size=320)     # bench.py's spread of the predicted scales
    w["hyper_synthesis/layer_2/bias"] = b.astype(np.float32)
    m.set_weights(w)
    return m


def test_model_decode_is_unchanged_and_encode_keeps_sigma(model, dev):
    from shallow_ntc_amd import ops
    from shallow_ntc_amd.common import data_lib
    from shallow_ntc_amd.graphs import DecodeGraph
    codes, want = [], []
    assert ops.MEAN_ONLY_HYPER
    try:
        for n, h, w in ((2, 128, 192), (1, 64, 64)):
            x = torch.from_numpy(data_lib.normalize_image(data_lib.synthetic_images(n, h, w, seed=7 + n))).to(dev)
            ops.MEAN_ONLY_HYPER = True
            on = model.encode(x)
            ops.LAUNCH_LOG = []
            px_on = model.decode(on[0], on[1], (h, w))
            log, ops.LAUNCH_LOG = ops.LAUNCH_LOG, None
            assert sum(isinstance(p, ops.ConvPlanColumns) and p.cout == 320 for p, *_ in log) == 1      # the path under test did run
            ops.MEAN_ONLY_HYPER = False
            off = model.encode(x)
            ops.LAUNCH_LOG = []
            px_off = model.decode(off[0], off[1], (h, w))
            log, ops.LAUNCH_LOG = ops.LAUNCH_LOG, None
            assert not any(isinstance(p, ops.ConvPlanColumns) for p, *_ in log)
            for a, b in zip(on, off):                   # (z_hat, symbols, bits_z, bits_y): encode still sees sigma
                assert torch.equal(a, b)
            assert px_on.dtype == torch.uint8 and torch.equal(px_on, px_off)
            codes.append((on[0], on[1], (h, w)))
            want.append(px_off)
        outs_off = model.decode_set(codes)
        ops.MEAN_ONLY_HYPER = True
        outs_on = model.decode_set(codes)
        for got_on, got_off, ref in zip(outs_on, outs_off, want):
            assert torch.equal(got_on, ref) and torch.equal(got_off, ref)
        # roofline bookkeeping: the entry's `flops` stays the layer's algorithmic count (the reference's table, which
        # tests/test_hip_fullsize.py sums), `launched_flops` is what the limited launch multiplies: half of it
        ops.PROFILE = []
        model.decode(*codes[0])
        prof, ops.PROFILE = ops.PROFILE, None
        lim = [e for e in prof if e["kind"] == "convT" and e["cin"] == 480]
        assert len(lim) == 1 and lim[0]["cout"] == 320 and lim[0]["flops"] == 2 * lim[0]["launched_flops"]
        assert all(e["flops"] == e["launched_flops"] for e in prof if e is not lim[0] and "launched_flops" in e)
        z, s, hw = codes[1]
        graph = DecodeGraph(model, z, s, hw)
        assert torch.equal(graph(), want[1])
        assert torch.equal(graph(z, s), want[1])
    finally:
        ops.MEAN_ONLY_HYPER, ops.LAUNCH_LOG, ops.PROFILE = True, None, None


def test_tuning_round_trip_keeps_view_and_parent_apart(dev):
    from shallow_ntc_amd import ops
    rng = np.random.default_rng(11)
    base = len(ops._PLAN_REGISTRY)
    plan = ops.ConvPlan("convT", dev_t(rng.standard_normal((3, 3, 192, 96)) * 0.05, dev), None, 1)
    assert len(ops._PLAN_REGISTRY) == base + 1
    view = plan.columns(96)
    assert plan.columns(96) is view and len(ops._PLAN_REGISTRY) == base + 1          # a view is no plan of its own
    n, h, w = 2, 12, 20
    x = dev_t(rng.standard_normal((n, h, w, 96)), dev)
    full = plan(x)
    model_view, model_full = view.launch_info(n, h, w), plan.launch_info(n, h, w)
    pick_view = [c for c in view.candidates(n, h, w) if c[0] != model_view[0]][0]
    pick_full = [c for c in plan.candidates(n, h, w) if c[0] not in (model_full[0], pick_view[0])][0]
    view.set_choice(n, h, w, *pick_view)
    plan.set_choice(n, h, w, *pick_full)
    tuned_view, tuned_full = view.launch_info(n, h, w), plan.launch_info(n, h, w)
    assert tuned_view[0] == pick_view[0] and tuned_full[0] == pick_full[0]
    entries = [e for e in ops.export_tuning() if e[0] == base]
    assert sorted(e[1:7] for e in entries) == [("convT", 96, 96, n, h, w), ("convT", 96, 192, n, h, w)]
    assert all(len(e) == 9 for e in entries)
    plan.clear_tuning()
    assert view._tuned == {} and plan._tuned == {}
    assert view.launch_info(n, h, w) == model_view and plan.launch_info(n, h, w) == model_full
    # the view's entry alone: the parent's full-width launch at the same (n, h, w) stays the cost model's
    assert ops.import_tuning([e for e in entries if e[3] == 96], strict=True) == 1
    assert view.launch_info(n, h, w) == tuned_view and plan.launch_info(n, h, w) == model_full
    assert ops.import_tuning(entries, strict=True) == 2
    assert view.launch_info(n, h, w) == tuned_view and plan.launch_info(n, h, w) == tuned_full
    assert view._tuned == {(n, h, w): pick_view} and plan._tuned == {(n, h, w): pick_full}
    view.drop_choice(n, h, w)               # one choice goes, the other stays
    assert view.launch_info(n, h, w) == model_view and plan.launch_info(n, h, w) == tuned_full
    assert torch.equal(view(x), full[..., :96].contiguous()) and torch.equal(plan(x), full)
    assert len(ops._PLAN_REGISTRY) == base + 1
