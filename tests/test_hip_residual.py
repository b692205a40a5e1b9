"""The coded pixel residual layer on the GPU (csrc/residual.hip, wire format 8, DESIGN.md 4.7 "residual layer"): the three kernels
against the numpy restatement of the rule (tests/residual_cases.py) in exact integers, the per-pixel guarantee end to end, the
composition with every way of making the base file, the exact table choice, the prediction against the file, the decode paths and
the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import residual_cases as rc
from oracle import rans_np
from test_hip_itinf_bitstream import hyper_model, images  # noqa: F401  (hyper_model: a fixture)

pytestmark = pytest.mark.gpu

N = 3
DELTAS = (0, 1, 2, 5, 127)
# 1 x 1 (every clamped neighbour is the pixel: a = 0), two pixels, 3 x 5 (w c = 15: the element-wise path, h w c % 4 != 0),
# 4 x 5 (16-byte units that run over a row's end), a tile, odd sizes, and one that takes several passes of several workgroups
SHAPES = [(1, 1), (1, 2), (2, 1), (3, 5), (4, 5), (16, 16), (17, 33), (65, 127), (300, 401)]


def dv(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def offset_view(t, elems):
    """The same values at an address ``elems`` elements past an aligned one: the kernels' element-wise path."""
    flat = torch.empty((t.numel() + elems,), dtype=t.dtype, device=t.device)
    view = flat[elems:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    return view


@pytest.fixture(scope="module")
def kernel_cases():
    """Per (h, w, c): x, base and the restatement's classes, computed once."""
    out = {}
    for h, w in SHAPES:
        for c in (3, 1):
            x, base = rc.images(N, h, w, c, seed=h * 1000 + w * 10 + c)
            out[h, w, c] = (x, base, rc.pixels(x), rc.classes(base))
    return out


def test_inputs_hold_what_they_claim(kernel_cases):
    x, base, x8, _ = kernel_cases[65, 127, 3]
    v = (x.astype(np.float32) + np.float32(0.5)) * np.float32(255.0)
    assert (np.abs(v - np.floor(v) - 0.5) == 0).sum() > 100            # exact k + 0.5 ties
    assert (x > 0.5).any() and (x < -0.5).any()
    r = x8 - base
    assert r.max() == 255 and r.min() == -255 and (base == 0).any() and (base == 255).any()


@pytest.mark.parametrize("c", [3, 1])
@pytest.mark.parametrize("h,w", SHAPES)
def test_kernels_against_the_restatement(dev, kernel_cases, h, w, c):
    from shallow_ntc_amd import entropy_coding as ec
    x, base, x8, cls = kernel_cases[h, w, c]
    E = h * w * c
    if (h, w, c) == (300, 401, 3):                                   # several passes of several workgroups, by a non-multiple
        for per_unit in (ec.RESIDUAL_VEC, 1):
            units = E // per_unit
            grid = min(-(-units // ec.RESIDUAL_THREADS), max(1, ec.RESIDUAL_GRID // N))
            assert E % ec.RESIDUAL_VEC == 0 and grid > 1 and units > grid * ec.RESIDUAL_THREADS and units % (grid * ec.RESIDUAL_THREADS) != 0
    xd, bd = dv(x, dev), dv(base, dev)
    xu, bu = offset_view(xd, 1), offset_view(bd, 1)
    rng = np.random.default_rng(E)
    choice = rng.integers(0, 64, size=(N, 8 * c)).astype(np.uint8)
    choice[0, :2] = (63, 0)
    ids = ec.residual_table_ids(bd, dv(choice, dev))
    assert (ids.cpu().numpy() == rc.table_ids(cls, choice)).all()
    assert torch.equal(ec.residual_table_ids(bu, dv(choice, dev)), ids)
    for delta in DELTAS:
        want_q = rc.quantize(x8, base, delta)
        q, hist = ec.residual_quantize(xd, bd, delta)
        assert (q.cpu().numpy() == want_q).all(), delta
        hist_h = hist.cpu().numpy().view(np.uint32)
        assert (hist_h == rc.histogram(want_q, cls, c)).all() and int(hist_h.sum()) == N * E, delta
        qu, hu = ec.residual_quantize(xu, bu, delta)                 # V = 1: the same integers
        assert torch.equal(qu, q) and torch.equal(hu, hist), delta
        out, count = ec.residual_apply(bd, q, delta)
        want = rc.reconstruct(base, want_q, delta)
        assert (out.cpu().numpy() == want).all() and int(count.item()) == 0, delta
        assert int(np.abs(want - x8).max()) <= delta
        # any int32 decodes: values no encoder writes are clipped and counted
        bad_q = want_q.copy().reshape(-1)
        at = rng.choice(bad_q.size, size=min(5, bad_q.size), replace=False)
        bad_q[at] = np.resize([rc.q_max(delta) + 1, -rc.q_max(delta) - 1, 2 ** 31 - 1, -2 ** 31, 256], len(at))
        bad_q = bad_q.reshape(want_q.shape)
        qd = dv(bad_q.astype(np.int32), dev)
        out, count = ec.residual_apply(bd, qd, delta)
        assert (out.cpu().numpy() == rc.reconstruct(base, bad_q, delta)).all() and int(count.item()) == len(at), delta
        ou, cu = ec.residual_apply(bu, offset_view(qd, 1), delta)
        assert torch.equal(ou, out) and int(cu.item()) == len(at), delta


def test_kernels_refuse_before_any_launch(dev):
    """Null pointers, max_error outside 0 .. 127, c outside 1 .. 4 and non-positive sizes: SNTC_ERR_BAD_SHAPE, outputs untouched."""
    from shallow_ntc_amd import _capi as capi
    from shallow_ntc_amd import ops
    lib = capi.load()
    n, h, w, c = 2, 4, 6, 3
    x = torch.zeros((n, h, w, 4), dtype=torch.float32, device=dev)
    base = torch.zeros((n, h, w, 4), dtype=torch.uint8, device=dev)
    choice = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    q = torch.full((n, h, w, 4), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    hist = torch.full((n, 32, 511), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    ids = torch.full((n, h, w, 4), 0x5A5A, dtype=torch.int16, device=dev)
    out = torch.full((n, h, w, 4), 0x5A, dtype=torch.uint8, device=dev)
    count = torch.full((1,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    s = ops._stream()
    sizes = [(0, h, w, c), (-1, h, w, c), (n, 0, w, c), (n, h, -3, c), (n, h, w, 0), (n, h, w, 5), (65536, h, w, c), (n, 1 << 16, 1 << 15, 1)]
    calls = []
    for a in sizes:
        calls += [lambda a=a: lib.sntc_residual_quantize(p(x), p(base), *a, 1, p(q), p(hist), s),
                  lambda a=a: lib.sntc_residual_table_ids(p(base), p(choice), *a, p(ids), s),
                  lambda a=a: lib.sntc_residual_apply(p(base), p(q), *a, 1, p(out), p(count), s)]
    for d in (-1, 128, 255):
        calls += [lambda d=d: lib.sntc_residual_quantize(p(x), p(base), n, h, w, c, d, p(q), p(hist), s),
                  lambda d=d: lib.sntc_residual_apply(p(base), p(q), n, h, w, c, d, p(out), p(count), s)]
    for k in range(4):
        args = [x, base, q, hist]
        args[k] = None
        calls.append(lambda args=args: lib.sntc_residual_quantize(p(args[0]), p(args[1]), n, h, w, c, 1, p(args[2]), p(args[3]), s))
        args = [base, q, out, count]
        args[k] = None
        calls.append(lambda args=args: lib.sntc_residual_apply(p(args[0]), p(args[1]), n, h, w, c, 1, p(args[2]), p(args[3]), s))
    for k in range(3):
        args = [base, choice, ids]
        args[k] = None
        calls.append(lambda args=args: lib.sntc_residual_table_ids(p(args[0]), p(args[1]), n, h, w, c, p(args[2]), s))
    for call in calls:
        assert call() == capi.ERR_BAD_SHAPE
    torch.cuda.synchronize()
    assert (q == 0x5A5A5A5A).all() and (hist == 0x5A5A5A5A).all() and (ids == 0x5A5A).all() and (out == 0x5A).all()
    assert int(count.item()) == 0x5A5A5A5A
    assert lib.sntc_residual_quantize(p(x), p(base), n, h, w, 4, 0, p(q), p(hist), s) == capi.OK      # c = 4 is served: 64 KB of LDS
    assert (q == 128).all() and int(hist.sum().item()) == n * h * w * 4      # x = 0 is pixel rint(127.5) = 128 over base 0


# -- the codec ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batches(dev):
    return [images(2, 64, 64, dev), images(1, 70, 90, dev, seed=5)]


def x8_of(x):
    return rc.pixels(x.cpu().numpy())


@pytest.mark.parametrize("delta", [0, 1, 3])
def test_every_pixel_is_within_the_bound(hyper_model, batches, delta):
    from shallow_ntc_amd import entropy_coding as ec
    for x in batches:
        blob = hyper_model.compress(x, max_error=delta)
        assert blob[4] == 8
        x8 = x8_of(x)
        out = hyper_model.decompress(blob).cpu().numpy().astype(np.int64)
        worst = int(np.abs(out - x8).max())
        assert worst <= delta, (worst, delta)
        if delta == 0:
            assert (out == x8).all()
        base = hyper_model.decompress(ec.split_residual(blob)[0]).cpu().numpy().astype(np.int64)
        assert int(np.abs(base - x8).max()) > delta                   # the base alone does not keep the promise
        report = hyper_model.last_compress_report
        assert len(report) == x.shape[0] and all(r["max_error"] == delta and len(r["residual_tables"]) == 24 for r in report)
        assert [r["residual_bits_predicted"] for r in report] == hyper_model.residual_bits(x, ec.split_residual(blob)[0], delta).tolist()


def test_composition_with_every_base(hyper_model, batches):
    from shallow_ntc_amd import entropy_coding as ec
    x = batches[0]
    h, w = hyper_model.step_offsets_shape(64, 64)
    offs = np.zeros((2, h, w), np.int8)
    offs[:, :, w // 2:] = 6
    for a, version in (({}, 3), (dict(step=4), 5), (dict(step_offsets=offs), 7), (dict(target_bpp=0.5), None)):
        plain = hyper_model.compress(x, **a)
        assert version is None or plain[4] == version
        layered = hyper_model.compress(x, max_error=2, **a)
        report = hyper_model.last_compress_report
        assert ec.split_residual(layered)[0] == plain, a
        assert layered == hyper_model.add_residual(plain, x, 2), a
        assert all(r["max_error"] == 2 for r in report) and ("step_chosen" in report[0]) == ("target_bpp" in a)
        assert int(np.abs(hyper_model.decompress(layered).cpu().numpy().astype(np.int64) - x8_of(x)).max()) <= 2


def test_the_choice_is_exact(hyper_model, batches):
    from shallow_ntc_amd import entropy_coding as ec
    codec = hyper_model._get_codec()
    x = batches[0]
    plain = hyper_model.compress(x)
    for delta in (0, 2):
        codec.add_residual(plain, x, delta)
        last = codec.last_residual
        base = hyper_model.decompress(plain)
        q, hist = ec.residual_quantize(x, base, delta)
        assert (hist.cpu().numpy().view(np.uint32) == last["hist"]).all()
        ids = ec.residual_table_ids(base, dv(last["choice"], base.device))
        cost = ec.rans_cost(q.view(2, -1), ids.view(2, -1), codec.y_tables).cpu().numpy()
        assert cost.tolist() == last["cost_q"].tolist() and last["cost_q"].dtype == np.int64
        price = rc.prices(ec.normal_tables(), ec.cost_table)
        total = last["hist"].astype(np.int64) @ price.T              # [n, 24, 64]
        best = total.min(axis=2)
        chosen = np.take_along_axis(total, last["choice"].astype(np.int64)[..., None], axis=2)[..., 0]
        assert (chosen == best).all() and (last["choice"] == total.argmin(axis=2)).all()
        assert (last["hist"].sum(axis=2) > 0).sum() > 6               # several classes are in use


def test_prediction_against_the_file(hyper_model, dev, monkeypatch):
    """Per stream, payload bits = cost / 65536 + 32 per lane + the coder's renormalisation slack (no closed form).  The bar is
    taken the way test_file_payload_against_the_cost takes it: twice the largest |gap| the pure-Python restatement of the format
    shows on this test's own symbols, at least 16 bits per lane.  Per image the costs and lane states sum to ``residual_bits``,
    exactly.  Measured on the two 38 400-value streams of a 160 x 160 image (64 lanes): payload - predicted = -351 and -410 bits
    at max_error 0, -246 and -319 bits at max_error 2, the GPU's streams and the restatement's to the bit (negative: a final
    state holds up to 16 bits less than the 32 counted for it); the bar is 2 x 410 = 820 bits against 1024 = 16 per lane."""
    from shallow_ntc_amd import entropy_coding as ec
    codec = hyper_model._get_codec()
    x = images(1, 160, 160, dev, seed=9)
    plain = hyper_model.compress(x)
    memo = {}
    cdf = rans_np._cdf
    monkeypatch.setattr(rans_np, "_cdf", lambda f: memo.setdefault(id(f), cdf(f)))
    tabs = ec.normal_tables()
    ltabs = [(lo, [int(v) for v in f]) for lo, f in tabs]
    price = rc.prices(tabs, ec.cost_table)
    for delta in (0, 2):
        blob = hyper_model.add_residual(plain, x, delta)
        _, info = ec.split_residual(blob)
        segments, lanes = info["segments"], info["lanes"]
        assert (segments, lanes) == (2, 64)
        base = hyper_model.decompress(plain)
        q = ec.residual_quantize(x, base, delta)[0].cpu().numpy().reshape(-1).astype(np.int64)
        ids = ec.residual_table_ids(base, dv(info["choice"], dev)).cpu().numpy().reshape(-1).astype(np.int64)
        E = q.size
        eseg = -(-(-(-E // segments)) // 64) * 64
        ideal, gaps, refs = [], [], []
        for s in range(segments):
            lo, hi = s * eseg, min((s + 1) * eseg, E)
            ideal.append(int(price[ids[lo:hi], q[lo:hi] + 255].sum()) / 65536.0 + 32 * lanes)
            gaps.append(16 * int(info["lens"][s]) - ideal[-1])
            refs.append(16 * len(rans_np.encode_stream(q[lo:hi], ids[lo:hi], ltabs, lanes)) - ideal[-1])
        predicted = hyper_model.residual_bits(x, plain, delta)
        assert predicted.shape == (1,) and predicted[0] == sum(ideal)
        worst = max(abs(r) for r in refs)
        print(f"\nresidual layer, max_error {delta}: payload - predicted per stream, gpu {gaps}, restatement {refs}")
        for g in gaps:
            assert abs(g) <= max(2 * worst, 16 * lanes), (g, worst)
    both = hyper_model.residual_bits(x, plain, [0, 2, 5])
    assert both.shape == (1, 3) and both[0, 1] == predicted[0] and both[0, 0] > both[0, 1] > both[0, 2]


def test_decode_paths(hyper_model, batches, dev):
    from shallow_ntc_amd import _capi as capi
    from shallow_ntc_amd import entropy_coding as ec
    a = hyper_model.compress(batches[0], max_error=1)
    plain = hyper_model.compress(images(1, 48, 80, dev, seed=3))
    b = hyper_model.compress(batches[1], max_error=0)
    alone = [hyper_model.decompress(t) for t in (a, plain, b)]
    for order in ((0, 1, 2), (2, 1, 0)):
        blobs = [(a, plain, b)[k] for k in order]
        for got, k in zip(hyper_model.decompress_many(blobs), order):
            assert torch.equal(got, alone[k]), order
    _, info = ec.split_residual(a)
    raw = bytearray(a)
    raw[info["pos"] + 2 * (info["words"] // 2)] ^= 0x10               # a word of the residual payload
    with pytest.raises(capi.SntcError, match="corrupt"):
        hyper_model.decompress(bytes(raw))
    with pytest.raises(capi.SntcError, match="corrupt"):
        hyper_model.decompress_many([plain, bytes(raw)])
    base_blob = ec.split_residual(a)[0]
    hd = hyper_model._get_codec()._parse(base_blob)
    raw = bytearray(a)
    raw[12 + hd["pos"] + 2 * (hd["zw"] + hd["yw"] // 2)] ^= 0x10      # a word of the base's y payload (12: the v8 header)
    with pytest.raises(capi.SntcError, match="corrupt"):
        hyper_model.decompress(bytes(raw))


def test_model_refusals(hyper_model, batches, dev):
    from shallow_ntc_amd.mshyper import configs
    from shallow_ntc_amd.mshyper.models import Model
    x = batches[0]
    layered = hyper_model.compress(x, max_error=1)
    with pytest.raises(ValueError, match="split_residual"):
        hyper_model.transcode(layered, shift=1)
    with pytest.raises(ValueError, match="split_residual"):
        hyper_model.add_residual(layered, x, 0)
    with pytest.raises(ValueError, match="split_residual"):
        hyper_model.residual_bits(x, layered, 0)
    with pytest.raises(ValueError, match="max_error"):
        hyper_model.compress(x, max_error=128)
    with pytest.raises(ValueError, match="decodes to"):
        hyper_model.add_residual(hyper_model.compress(x), batches[1], 1)
    split = Model(device=dev, precision="bf16x3", **configs.two_layer_syn(rd_lambda=0.02))
    with pytest.raises(NotImplementedError, match="bf16x3"):
        split.compress(x, max_error=1)
    with pytest.raises(NotImplementedError, match="bf16x3"):
        split.add_residual(split.compress(x), x, 1)
