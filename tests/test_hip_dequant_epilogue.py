"""The dequantising epilogue of column-limited gather-GEMM launches (sntc_conv_forward_columns_dequant,
``plan.columns(ncols)(x, symbols=...)``, ops.FUSE_DEQUANT): y_hat = v + (float)symbols leaves the launch that computes v, and is
THE SAME BITS as the two launches it replaces -- every case asserts
``torch.equal(fused, ops.dequant_mean(symbols, plan.columns(ncols)(x)))``.

The epilogue is applied in four places, and every one is reached here:
  1. the staged 16-byte path of a tile computed by one workgroup (static schedule, every tile variant the decode uses);
  2. the same path of a stream-K tile that its second owner finishes from the first owner's published accumulators;
  3. the split-K finish kernel (gg_reduce_kernel), which applies it through the scalar form (apply_epilogue1);
  4. (the scalar path of gg_kernel itself serves outputs whose channel count is no multiple of 4: a column-limited launch never
     has one, ncols % 4 == 0.)
Symbols are random in [-40, 40] with 0, +-1 and the integers around 2^24 planted (where int32 -> float32 starts to round)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PLANTED = [0, 1, -1, (1 << 24) - 1, -((1 << 24) - 1), 1 << 24, -(1 << 24), (1 << 24) + 1, -((1 << 24) + 1)]
# (variant, column-major unit order): 128 x 32, 128 x 64, 128 x 96, 128 x 128 (one wave row of four tiles; 2 x 2 waves in both
# unit orders), 64 x 64
TILES = [(1, False), (2, False), (3, False), (4, False), (9, False), (9, True), (8, False)]


def dev_t(a, dev, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev)


def make_symbols(shape, seed, dev):
    """int32 in [-40, 40]; the planted values at the first and the last positions and at every 997th in between."""
    rng = np.random.default_rng(seed)
    s = rng.integers(-40, 41, size=shape, dtype=np.int64).astype(np.int32)
    flat = s.reshape(-1)
    k = len(PLANTED)
    flat[:k] = PLANTED
    flat[-k:] = PLANTED
    idx = np.arange(k, flat.size - k, 997)
    flat[idx] = np.resize(np.array(PLANTED, np.int32), idx.size)
    return dev_t(s, dev, np.int32)


_LAYERS = {}


def layer(cin, cout, ncols, n, h, w, dev):
    """One transposed 3x3 / 1 layer, its input, symbols, and the two-launch reference under the plan's own schedule (computed
    once per shape, shared, never modified)."""
    from shallow_ntc_amd import ops
    key = (cin, cout, ncols, n, h, w)
    if key not in _LAYERS:
        rng = np.random.default_rng(1000 * cin + 10 * n + h)
        wk = (rng.standard_normal((3, 3, cout, cin)) / np.sqrt(9 * cin / 4)).astype(np.float32)
        b = rng.standard_normal(cout).astype(np.float32)
        plan = ops.ConvPlan("convT", dev_t(wk, dev), dev_t(b, dev), 1)
        x = dev_t(rng.standard_normal((n, h, w, cin)), dev)
        sym = make_symbols((n, h, w, ncols), cin + n + h, dev)
        want = ops.dequant_mean(sym, plan.columns(ncols)(x))
        _LAYERS[key] = dict(plan=plan, x=x, sym=sym, want=want)
    return _LAYERS[key]


class forced:
    """Restores the plan's forced tile and schedule; a timed-out stream-K hand-off fails the test."""

    def __init__(self, plan):
        self.plan = plan

    def __enter__(self):
        return self.plan

    def __exit__(self, *exc):
        from shallow_ntc_amd import ops
        self.plan.set_tile(0)
        self.plan.set_stream_k(True)
        if exc[0] is None:
            ops.check_conv_status()
        else:
            ops.take_conv_status()
        return False


def test_reference_is_symbols_plus_mu(dev):
    """The two-launch reference itself: float32(symbols) + mu, the conversion rounding to nearest even past 2^24."""
    L = layer(32, 64, 32, 1, 5, 7, dev)
    mu = L["plan"].columns(32)(L["x"])
    assert torch.equal(L["want"], L["sym"].to(torch.float32) + mu)
    assert float(torch.tensor((1 << 24) + 1, dtype=torch.int32).to(torch.float32)) == float(1 << 24)


@pytest.mark.parametrize("shape", [(1, 5, 7), (3, 16, 24)], ids=lambda s: "x".join(map(str, s)))
def test_cost_model_schedule(shape, dev):
    """3x3 / 1 transposed, 32 -> 64, the first 32 columns: 35 rows (one ragged tile) and 1152 rows (several tiles)."""
    from shallow_ntc_amd import ops
    n, h, w = shape
    L = layer(32, 64, 32, n, h, w, dev)
    view = L["plan"].columns(32)
    got = view(L["x"], symbols=L["sym"])
    assert got.shape == L["want"].shape and got.dtype == torch.float32 and got.is_contiguous()
    assert torch.equal(got, L["want"])
    assert torch.equal(ops.dequant_mean(L["sym"], view(L["x"])), L["want"])      # the same view still stores plainly when asked to


@pytest.mark.parametrize("tile", TILES, ids=lambda t: f"v{t[0]}{'colm' if t[1] else ''}")
@pytest.mark.parametrize("shape", [(1, 5, 7), (3, 16, 24)], ids=lambda s: "x".join(map(str, s)))
def test_every_decode_tile_one_workgroup_per_tile(shape, tile, dev):
    n, h, w = shape
    v, colm = tile
    L = layer(32, 64, 32, n, h, w, dev)
    view = L["plan"].columns(32)
    with forced(L["plan"]) as plan:
        plan.set_tile(v)
        if colm:      # the column-major twin is a stream-K instance: forced, it runs whole tiles where the launch is too small to cut
            plan.set_stream_k(True, dma=False, force=True, colm=True)
        else:
            plan.set_stream_k(False, dma=False)
        assert view.launch_info(n, h, w)[0] == v
        assert torch.equal(view(L["x"], symbols=L["sym"]), L["want"]), tile


@pytest.mark.parametrize("tile", TILES, ids=lambda t: f"v{t[0]}{'colm' if t[1] else ''}")
def test_every_decode_tile_stream_k_second_owner(tile, dev):
    """4 x 127 x 132 = 67056 rows, 18 stages per tile: 524 tiles of 128 rows, 1048 of 64.  The workers are a multiple of 8 no larger
    than the tile count, so forced stream-K runs on fewer workgroups than there are tiles: shares end inside tiles, and those
    tiles are finished -- epilogue included -- by their second owner."""
    n, h, w = 4, 127, 132
    v, colm = tile
    L = layer(32, 64, 32, n, h, w, dev)
    view = L["plan"].columns(32)
    with forced(L["plan"]) as plan:
        plan.set_tile(v)
        plan.set_stream_k(False, dma=False)
        assert view.launch_info(n, h, w)[0] == v
        nb_static = view.launch_info(n, h, w)[1]
        assert torch.equal(view(L["x"], symbols=L["sym"]), L["want"]), (tile, "static")
        plan.set_stream_k(True, dma=False, force=True, colm=colm)
        v_sk, nb_sk = view.launch_info(n, h, w)
        print(f"variant {v}{' colm' if colm else ''}: {nb_sk} stream-K workgroups, {nb_static} tiles")
        assert v_sk == v and view.launch_order(n, h, w) == colm
        assert nb_sk < nb_static and nb_static % nb_sk != 0, (nb_sk, nb_static)
        assert torch.equal(view(L["x"], symbols=L["sym"]), L["want"]), (tile, "stream-K")


def test_split_k_finish(dev):
    """3x3, 256 -> 64, the first 32 columns at 1 x 8 x 12: 144 stages on one row tile, which pick_ksplit cuts into K ranges --
    the launch has more workgroups than any tiling of 96 rows x 32 columns has tiles (two, of 64 rows) and needs the slabs --
    so the epilogue runs in gg_reduce_kernel."""
    from shallow_ntc_amd import _capi as capi
    n, h, w = 1, 8, 12
    L = layer(256, 64, 32, n, h, w, dev)
    view = L["plan"].columns(32)
    v, nb = view.launch_info(n, h, w)
    # A split-K launch's workspace is exactly ksplit slabs of rows x columns floats (a stream-K one's is slabs of a whole tile
    # plus a flag per worker), and its grid is tiles x ksplit.  96 rows x 32 columns are one tile of 128 rows or two of 64,
    # whichever variant the cost model picks, so both facts together say that K was cut and gg_reduce_kernel finishes the launch.
    slab = 96 * 32 * 4
    ws = int(capi.load().sntc_conv_columns_workspace_bytes(L["plan"]._h, n, h, w, 32))
    ksplit = ws // slab
    print(f"variant {v}: {nb} workgroups, workspace {ws} B = {ksplit} slabs")
    assert ws == ksplit * slab and ksplit > 1, (v, nb, ws)
    assert nb in (ksplit, 2 * ksplit), (v, nb, ksplit)
    assert torch.equal(view(L["x"], symbols=L["sym"]), L["want"])


def test_refusals_come_before_any_launch(dev):
    from shallow_ntc_amd import _capi as capi
    from shallow_ntc_amd import ops
    L = layer(32, 64, 32, 1, 5, 7, dev)
    plan, x = L["plan"], L["x"]
    lib = capi.load()
    y = torch.full((1, 5, 7, 68), 7.0, device=dev)
    sym = torch.zeros((1, 5, 7, 68 + 4), dtype=torch.int32, device=dev)
    ws = torch.empty((1 << 20,), device=dev)

    def launch(p, ncols, s):
        return lib.sntc_conv_forward_columns_dequant(p._h, x.data_ptr(), 1, 5, 7, ncols, s, y.data_ptr(), ws.data_ptr(), ws.numel() * 4,
                                                     None)

    assert sym.data_ptr() % 16 == 0
    for ncols in (0, 30, plan.cout + 4):                       # what sntc_conv_forward_columns refuses
        assert launch(plan, ncols, sym.data_ptr()) == capi.ERR_UNSUPPORTED
    for off in (4, 8, 12):                                     # a misaligned symbols pointer
        assert launch(plan, 32, sym.data_ptr() + off) == capi.ERR_UNSUPPORTED
    assert launch(plan, 32, None) == capi.ERR_UNSUPPORTED
    rng = np.random.default_rng(3)
    up2 = ops.ConvPlan("convT", dev_t(rng.standard_normal((5, 5, 64, 32)) * 0.05, dev), None, 2)       # several phase groups
    bf3 = ops.ConvPlan("convT", dev_t(rng.standard_normal((3, 3, 64, 32)) * 0.05, dev), None, 1, bf16x3=True)
    add = ops.ConvPlan("convT", dev_t(rng.standard_normal((3, 3, 64, 32)) * 0.05, dev), None, 1, epilogue=capi.EPI_ADD)
    for p in (up2, bf3, add):
        assert launch(p, 32, sym.data_ptr()) == capi.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())           # nothing was written
    # the Python forms: symbols belong to a column view, have the output's shape, and are int32
    view = plan.columns(32)
    with pytest.raises(capi.SntcError):
        plan(x, symbols=torch.zeros((1, 5, 7, 64), dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        view(x, symbols=torch.zeros((1, 5, 7, 64), dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        view(x, symbols=torch.zeros((1, 5, 7, 32), dtype=torch.int64, device=dev))
    with pytest.raises(capi.SntcError):            # a plan may not be BUILT with the override's epilogue
        ops.ConvPlan("convT", dev_t(rng.standard_normal((3, 3, 64, 32)) * 0.05, dev), None, 1, epilogue=9)


@pytest.fixture(scope="module")
def model(dev):
    from shallow_ntc_amd.mshyper import configs
    from shallow_ntc_amd.mshyper.models import Model
    return Model(device=dev, **configs.two_layer_syn(rd_lambda=0.005))


def test_model_decode_same_pixels_without_the_dequant_launch(model, dev, monkeypatch):
    """``Model.decode`` and ``decode_set`` on 2 images of 64 x 128: equal uint8 pixels with ops.FUSE_DEQUANT on and off; the fused
    run's hyper-synthesis launch carries the dequantisation (ops.PROFILE, still kind "convT") and no dequant_kernel is launched
    (every product launch of it goes through ops.dequant_scale_normal, counted here)."""
    from shallow_ntc_amd import ops
    from shallow_ntc_amd.common import data_lib
    calls = []
    plain = ops.dequant_scale_normal
    monkeypatch.setattr(ops, "dequant_scale_normal", lambda *a, **k: (calls.append(1), plain(*a, **k))[1])
    x = torch.from_numpy(data_lib.normalize_image(data_lib.synthetic_images(2, 64, 128, seed=11))).to(dev)
    z_hat, sym = model.encode(x)[:2]
    x2 = torch.from_numpy(data_lib.normalize_image(data_lib.synthetic_images(1, 64, 64, seed=12))).to(dev)
    z2, sym2 = model.encode(x2)[:2]
    assert ops.FUSE_DEQUANT and ops.PROFILE is None
    out = {}
    try:
        for fuse in (True, False):
            ops.FUSE_DEQUANT = fuse
            del calls[:]
            ops.PROFILE = []
            px = model.decode(z_hat, sym, (64, 128))
            prof, ops.PROFILE = ops.PROFILE, None
            hs3 = [e for e in prof if e["kind"] == "convT" and e["cin"] == 480]
            assert len(hs3) == 1 and hs3[0]["cout"] == sym.shape[-1]
            assert hs3[0]["dequant"] == fuse and sum(bool(e.get("dequant")) for e in prof) == int(fuse)
            assert len(calls) == (0 if fuse else 1)
            assert px.dtype == torch.uint8 and tuple(px.shape) == (2, 64, 128, 3)
            del calls[:]
            both = model.decode_set([(z_hat, sym, (64, 128)), (z2, sym2, (64, 64))])
            assert len(calls) == (0 if fuse else 2)
            out[fuse] = (px, both)
    finally:
        ops.FUSE_DEQUANT, ops.PROFILE = True, None
    assert torch.equal(out[True][0], out[False][0])
    for a, b in zip(out[True][1], out[False][1]):
        assert torch.equal(a, b)
    assert torch.equal(out[True][1][0], out[True][0])
