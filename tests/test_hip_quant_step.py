"""Variable-rate bitstreams (-m gpu; DESIGN.md 4.7, "variable rate"): the quantisation-step kernels of csrc/quant_step.hip against
their NumPy restatement (integer / bit equality), the one-pass ladder cost against ``np_cost`` and ``rans_cost``, wire format v5
through compress / decompress, and rate control by ``target_bpp``."""
from fractions import Fraction

import ctypes as C
import numpy as np
import pytest
import torch

from test_hip_itinf_bitstream import (big_table_set, fact_model, flushed_bits, hyper_model, image_words, images,  # noqa: F401
                                      payload_bits, slack_bar)
from test_rans_cost_host import np_cost, ref_cost_table

pytestmark = pytest.mark.gpu

N = 3
STEPS = [-32, 5, 32]          # image 0: ids + 32 clamp at table 63; image 2: ids - 32 clamp at table 0
# elements per image around a wave, one workgroup pass (1024 threads x 4 elements) and many workgroups, at c = 4; at c = 320 the
# sizes of the same neighbourhoods that 320 divides (1, 3, 13 and 219 pixels)
CASES = [(E, 4, s) for E in (4, 60, 64, 68, 1020, 1024, 1028, 4096, 4100, 70000) for s in (4, 8)] + \
        [(E, 320, s) for E in (320, 960, 4160, 70080) for s in (320, 640)]
IDS = [f"E{E}-c{c}-stride{s}" for E, c, s in CASES]
LADDERS = [[-32], [0], [32], [-32, -7, 0, 9, 32], [-32, -20, -11, -5, -3, -2, -1, 0, 1, 2, 3, 6, 12, 19, 27, 32]]


def f32(v):
    return np.float32(v)


def np_step_symbols(y, mu, ids, ks):
    """The rule in float32 NumPy: s = rint((y - mu) * inv_step) (a float32 subtract, then a float32 multiply; rint = half to
    even), t = clip(t0 - k, 0, 63); ``ks`` one ladder index per image."""
    from shallow_ntc_amd import entropy_coding as ec
    inv = np.array([ec.step_size(-k) for k in ks], np.float32).reshape(-1, *([1] * (y.ndim - 1)))
    d = (y.astype(np.float32) - mu.astype(np.float32)).astype(np.float32)
    p = (d * inv).astype(np.float32)
    k = np.array(ks, np.int64).reshape(inv.shape)
    return np.rint(p).astype(np.int32), np.clip(ids.astype(np.int64) - k, 0, 63).astype(np.int16), p


def make_case(E, c, stride, seed=0):
    """y [3, hw, c], mu rows of ``stride`` floats (the columns past c hold a raw-sigma half that gives base ids over 0 .. 63 when
    stride == 2 c), base ids over 0 .. 63.  The values are spread as the widest table a step selects, with runs of escapes on
    both sides and elements whose scaled difference is an exact .5 tie."""
    from shallow_ntc_amd import entropy_coding as ec
    rng = np.random.default_rng(seed + 7 * E + c + stride)
    hw = E // c
    ids = rng.integers(0, 64, size=(N, hw, c)).astype(np.int16)
    order = np.array([v for pair in zip(range(32), range(63, 31, -1)) for v in pair])      # 0, 63, 1, 62, ...: both ends first
    ids.reshape(N, -1)[:, :min(64, E)] = order[:min(64, E)]                                # every id present where E allows
    rows = np.zeros((N, hw, stride), np.float32)
    rows[..., :c] = (rng.standard_normal((N, hw, c)) * 2.0).astype(np.float32)
    if stride == 2 * c:     # raw sigma whose exp rounds to the id: ln(id) (id 0: ln 0.2), so that scale_table_ids gives ``ids``
        rows[..., c:] = np.log(np.maximum(ids.astype(np.float64), 0.2)).astype(np.float32)
    else:
        rows[..., c:] = rng.standard_normal((N, hw, stride - c)).astype(np.float32)      # never read
    mu = rows[..., :c]
    sig = 0.11 * np.exp(ec.SCALE_FACTOR * ids.astype(np.float64))
    d = rng.standard_normal((N, hw, c)) * sig * np.where(rng.random((N, hw, c)) < 0.2, 3.5, 1.0)
    y = (mu.astype(np.float64) + d).astype(np.float32)
    flat_y, flat_mu = y.reshape(N, -1), np.ascontiguousarray(mu).reshape(N, -1)
    for b, k in enumerate(STEPS):
        step, inv = f32(ec.step_size(k)), f32(ec.step_size(-k))
        # escapes on both sides: symbols far outside every table (|s| ~ 5000 .. 30000 after scaling)
        ne = min(6, E // 2)
        far = (rng.integers(5000, 30000, ne) * np.where(np.arange(ne) % 2, -1.0, 1.0) * float(step)).astype(np.float32)
        flat_y[b, E - ne:] = flat_mu[b, E - ne:] + far
        # exact ties: y - mu = a float whose product with inv_step is m + .5 exactly (searched among neighbouring floats)
        placed = 0
        for m in (0, 1, 2, -1, -2, 7, -8, 100):
            if placed >= min(8, E // 2):
                break
            cand = f32((m + 0.5) * float(step))
            for _ in range(8):
                if f32(cand * inv) == f32(m + 0.5):
                    j = placed
                    base = f32(0.0) if j % 2 == 0 else f32(np.ldexp(np.rint(np.ldexp(float(flat_mu[b, j]), 2)), -2))
                    flat_mu[b, j] = base                 # mu on a coarse grid: y = mu + cand is exact, so is y - mu
                    flat_y[b, j] = f32(base + cand)
                    if f32(flat_y[b, j] - base) == cand:
                        placed += 1
                    break
                cand = np.nextafter(cand, f32(np.inf) if f32(cand * inv) < f32(m + 0.5) else f32(-np.inf))
    rows[..., :c] = flat_mu.reshape(N, hw, c)
    y = flat_y.reshape(N, hw, c)
    return dict(E=E, c=c, hw=hw, stride=stride, y=y, rows=rows, mu=rows[..., :c], ids=ids)


_cases = {}


def case_of(E, c, stride):
    """One input set and its NumPy reference per shape, shared by every test."""
    key = (E, c, stride)
    if key not in _cases:
        cs = make_case(E, c, stride)
        cs["sym"], cs["tid"], cs["scaled"] = np_step_symbols(cs["y"], cs["mu"], cs["ids"], STEPS)
        _cases[key] = cs
    return _cases[key]


def dv(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def dev_case(cs, dev):
    """-> (y [3, hw, 1, c], hyper [3, hw, 1, stride], ids) on the device, NHWC with w = 1."""
    return (dv(cs["y"], dev).unsqueeze(2), dv(cs["rows"], dev).unsqueeze(2), dv(cs["ids"], dev).unsqueeze(2))


@pytest.fixture(scope="module")
def normal(dev):
    from shallow_ntc_amd import entropy_coding as ec
    tabs = ec.normal_tables()
    return tabs, ec.DeviceTables(tabs, dev), ref_cost_table(tabs)


# ------------------------------------------------------------------ kernels ------------------------------------------------
@pytest.mark.parametrize("E,c,stride", CASES, ids=IDS)
def test_step_symbols_is_the_float32_rule(E, c, stride, dev):
    from shallow_ntc_amd import entropy_coding as ec
    from shallow_ntc_amd import ops
    cs = case_of(E, c, stride)
    y, hyper, ids = dev_case(cs, dev)
    _, inv, sh = ec.step_tensors(STEPS, dev)
    sym, tid = ops.step_symbols(y, hyper, ids, inv, sh)
    np.testing.assert_array_equal(sym.cpu().numpy().reshape(cs["sym"].shape), cs["sym"])
    np.testing.assert_array_equal(tid.cpu().numpy().reshape(cs["tid"].shape), cs["tid"])
    np.testing.assert_array_equal(ec.step_table_ids(ids, sh).cpu().numpy().reshape(cs["tid"].shape), cs["tid"])
    # the inputs exercise what they claim: both ends of the table ladder are clamped to, values escape on both sides of the
    # tables, and some scaled differences are exact ties
    assert (cs["ids"][0].astype(int) + 32 > 63).any() and (cs["ids"][2].astype(int) - 32 < 0).any()
    assert (cs["sym"] > 4096).any() and (cs["sym"] < -4096).any()
    frac = cs["scaled"] - np.floor(cs["scaled"])
    assert (frac == 0.5).reshape(N, -1).any(axis=1).all()


@pytest.mark.parametrize("E,c,stride", [k for k in CASES if k[2] == 2 * k[1]], ids=[i for i, k in zip(IDS, CASES) if k[2] == 2 * k[1]])
def test_step_zero_is_todays_quantisation(E, c, stride, dev):
    """k = 0: the symbols of sntc_entropy_scale_normal, the ids of sntc_scale_table_ids, the values of sntc_dequant_scale_normal
    / sntc_dequant_mean -- bit for bit."""
    from shallow_ntc_amd import entropy_coding as ec
    from shallow_ntc_amd import ops
    cs = case_of(E, c, stride)
    y, hyper, ids = dev_case(cs, dev)
    base = ec.scale_table_ids(hyper)
    assert torch.equal(base, ids)                        # the raw-sigma half of the rows was built to give these ids
    st, inv, sh = ec.step_tensors([0] * N, dev)
    assert st.tolist() == [1.0] * N and inv.tolist() == [1.0] * N
    y_hat0, _, sym0 = ops.entropy_scale_normal(y, hyper, want_symbols=True)
    sym, tid = ops.step_symbols(y, hyper, base, inv, sh)
    assert torch.equal(sym, sym0) and torch.equal(tid, base)
    mu = hyper[..., :c].contiguous()
    for h in (hyper, mu):
        got = ops.dequant_step(sym, h, st)
        assert torch.equal(got.view(torch.int32), ops.dequant_scale_normal(sym, h).view(torch.int32))
    assert torch.equal(got.view(torch.int32), y_hat0.view(torch.int32))


def round_f32(fr):
    """The float32 nearest to the exact Fraction (ties to even), without going through a float64 sum."""
    c = np.float32(float(fr))
    cands = [np.nextafter(c, f32(-np.inf)), c, np.nextafter(c, f32(np.inf))]
    best = min(cands, key=lambda v: (abs(Fraction(float(v)) - fr), int(np.float32(v).view(np.uint32)) & 1))
    return np.float32(best)


@pytest.mark.parametrize("E,c,stride", [(1028, 4, 4), (4100, 4, 8), (960, 320, 640), (70080, 320, 320)])
def test_dequant_step_is_one_rounding(E, c, stride, dev):
    """y_hat = the correctly rounded float32 of the exact mu + step * s (an fma: ONE rounding), on a few thousand elements."""
    from shallow_ntc_amd import entropy_coding as ec
    from shallow_ntc_amd import ops
    cs = case_of(E, c, stride)
    _, hyper, _ = dev_case(cs, dev)
    st = ec.step_tensors(STEPS, dev)[0]
    got = ops.dequant_step(dv(cs["sym"], dev).unsqueeze(2), hyper, st).cpu().numpy().reshape(N, -1)
    sym, mu = cs["sym"].reshape(N, -1), np.ascontiguousarray(cs["mu"]).reshape(N, -1)
    rng = np.random.default_rng(E)
    pick = np.unique(np.concatenate([np.arange(min(E, 400)), np.arange(max(E - 100, 0), E), rng.integers(0, E, 600)]))
    double_rounding = 0
    for b, k in enumerate(STEPS):
        step = Fraction(ec.step_size(k))
        want = np.array([round_f32(Fraction(float(mu[b, j])) + step * int(sym[b, j])) for j in pick], np.float32)
        np.testing.assert_array_equal(got[b, pick].view(np.uint32), want.view(np.uint32))
        two = (np.float32(ec.step_size(k)) * sym[b, pick].astype(np.float32)).astype(np.float32) + mu[b, pick]
        double_rounding += int((two.astype(np.float32).view(np.uint32) != want.view(np.uint32)).sum())
    print(f"\nE={E} c={c}: {3 * len(pick)} elements checked, a multiply + add would differ on {double_rounding}")
    assert double_rounding > 0                           # the chosen elements can tell an fma from two roundings


@pytest.mark.parametrize("E,c,stride", CASES, ids=IDS)
def test_ladder_cost_is_the_numpy_sum(E, c, stride, dev, normal):
    """Every [image, candidate] entry of the one-pass kernel = np_cost of the NumPy symbols and ids = rans_cost of the symbols
    and ids sntc_step_symbols writes, for 1, 5 and 16 candidates that include both ends of the ladder and 0."""
    from shallow_ntc_amd import entropy_coding as ec
    from shallow_ntc_amd import ops
    tabs, dt, q = normal
    cs = case_of(E, c, stride)
    y, hyper, ids = dev_case(cs, dev)
    seen = {}
    for ladder in LADDERS:
        got = ec.step_ladder_cost(y, hyper, ids, ladder, dt)
        assert got.dtype == torch.int64 and tuple(got.shape) == (N, len(ladder))
        got = got.cpu().numpy()
        for j, k in enumerate(ladder):
            if k not in seen:
                sym, tid, _ = np_step_symbols(cs["y"], cs["mu"], cs["ids"], [k] * N)
                want = np_cost(sym.reshape(N, -1), tid.reshape(N, -1), tabs, q)
                _, inv, sh = ec.step_tensors([k] * N, dev)
                dsym, dtid = ops.step_symbols(y, hyper, ids, inv, sh)
                assert ec.rans_cost(dsym, dtid, dt).cpu().numpy().tolist() == want.tolist(), k
                seen[k] = want
            assert got[:, j].tolist() == seen[k].tolist(), (ladder, k)
    # more candidates than one launch takes: chunks of 16
    whole = list(range(ec.STEP_MIN, ec.STEP_MAX + 1, 3)) + [0]
    got = ec.step_ladder_cost(y, hyper, ids, whole, dt).cpu().numpy()
    for j, k in enumerate(whole):
        if k in seen:
            assert got[:, j].tolist() == seen[k].tolist(), k


def offset_view(t, pad, dev):
    return torch.cat([torch.zeros(pad, dtype=t.dtype, device=dev), t.flatten()])[pad:].view(t.shape)


def test_ladder_cost_with_tables_beyond_the_lds_limit(dev):
    """Descriptors and costs read from global memory (84 tables; the ladder is their first 64): the same exact sums, from
    aligned tensors and from views 4 bytes into their allocation (the element-wise load path)."""
    from shallow_ntc_amd import entropy_coding as ec
    big = big_table_set()
    db, q = ec.DeviceTables(big, dev), ref_cost_table(big)
    ladder = LADDERS[3]
    for key in ((4100, 4, 8), (70080, 320, 320)):
        cs = case_of(*key)
        y, hyper, ids = dev_case(cs, dev)
        got = ec.step_ladder_cost(y, hyper, ids, ladder, db).cpu().numpy()
        y2, h2, i2 = offset_view(y, 1, dev), offset_view(hyper, 1, dev), offset_view(ids, 2, dev)
        assert y2.data_ptr() % 16 == 4 and h2.data_ptr() % 16 == 4 and i2.data_ptr() % 8 == 4
        got2 = ec.step_ladder_cost(y2, h2, i2, ladder, db).cpu().numpy()           # the element-wise load path, tables in memory
        for j, k in enumerate(ladder):
            sym, tid, _ = np_step_symbols(cs["y"], cs["mu"], cs["ids"], [k] * N)
            want = np_cost(sym.reshape(N, -1), tid.reshape(N, -1), big, q).tolist()
            assert got[:, j].tolist() == want, k
            assert got2[:, j].tolist() == want, k


def test_ladder_cost_from_an_offset_view(dev, normal):
    """y, mu and the ids each start 4 bytes into their allocation: the element-wise load path on sizes that would take the
    vector path, the same sums."""
    from shallow_ntc_amd import entropy_coding as ec
    tabs, dt, q = normal
    ladder = LADDERS[4]
    for key in ((4096, 4, 4), (4160, 320, 640)):
        cs = case_of(*key)
        y, hyper, ids = dev_case(cs, dev)
        want = ec.step_ladder_cost(y, hyper, ids, ladder, dt)
        y2, h2, i2 = offset_view(y, 1, dev), offset_view(hyper, 1, dev), offset_view(ids, 2, dev)
        assert y2.data_ptr() % 16 == 4 and h2.data_ptr() % 16 == 4 and i2.data_ptr() % 8 == 4
        for a, b, cc in ((y2, h2, i2), (y2, hyper, ids), (y, h2, ids), (y, hyper, i2)):
            assert torch.equal(ec.step_ladder_cost(a, b, cc, ladder, dt), want)


# (n, hw, c, stride): units per image (4 elements; 1 on the offset-view path) exceed what the launch's workgroups take in one
# pass, by a non-multiple, so threads run the loop several times and advance (pixel, unit in the pixel) by the launch's stride:
# with 300 images a launch has ONE workgroup per image (512 // n), stride 1024 units = 12 pixels + 64 units at c = 320 (the carry
# into the next pixel happens) and 3 pixels + 64 elements on the element-wise path; 5 and 3 images give 102 and 170 workgroups.
STRIDE_CASES = [(300, 2251, 4, 4), (300, 2251, 4, 8), (300, 41, 320, 320), (300, 41, 320, 640), (5, 2503, 320, 640), (3, 300011, 4, 8)]


@pytest.mark.parametrize("n,hw,c,stride", STRIDE_CASES, ids=[f"n{n}-hw{hw}-c{c}-stride{s}" for n, hw, c, s in STRIDE_CASES])
def test_ladder_cost_over_several_passes(n, hw, c, stride, dev, normal):
    """The grid-stride advance of the ladder kernel, on both load paths: np_cost of the NumPy symbols = rans_cost of
    sntc_step_symbols' output = every entry of the one-pass launch, from aligned tensors and from views 4 bytes into theirs."""
    from shallow_ntc_amd import entropy_coding as ec
    from shallow_ntc_amd import ops
    tabs, dt, q = normal
    for per_unit in (4, 1):
        units = hw * c // per_unit
        grid = min(-(-units // 1024), max(1, 512 // n))
        assert units > grid * 1024 and units % (grid * 1024) != 0 and (per_unit == 4 or units > 2 * grid * 1024)
    rng = np.random.default_rng(n + hw + c + stride)
    ids = rng.integers(0, 64, size=(n, hw, c)).astype(np.int16)
    rows = (rng.standard_normal((n, hw, stride)) * 2.0).astype(np.float32)
    sig = 0.11 * np.exp(ec.SCALE_FACTOR * ids.astype(np.float64))
    y = (rows[..., :c] + rng.standard_normal((n, hw, c)) * sig * np.where(rng.random((n, hw, c)) < 0.2, 3.5, 1.0)).astype(np.float32)
    y.reshape(n, -1)[:, -4:] += np.array([20000.0, -20000.0, 300.0, -300.0], np.float32)         # escapes in the last pass
    mu = rows[..., :c]
    yd, hd, idd = (dv(a, dev).unsqueeze(2) for a in (y, rows, ids))
    ladder = [-32, -3, 0, 5, 32]
    want = []
    for k in ladder:
        sym, tid, _ = np_step_symbols(y, mu, ids, [k] * n)
        want.append(np_cost(sym.reshape(n, -1), tid.reshape(n, -1), tabs, q))
        _, inv, sh = ec.step_tensors([k] * n, dev)
        dsym, dtid = ops.step_symbols(yd, hd, idd, inv, sh)
        assert ec.rans_cost(dsym, dtid, dt).cpu().numpy().tolist() == want[-1].tolist(), k
    want = np.stack(want, axis=1)
    np.testing.assert_array_equal(ec.step_ladder_cost(yd, hd, idd, ladder, dt).cpu().numpy(), want)
    off = lambda t, pad: torch.cat([torch.zeros(pad, dtype=t.dtype, device=dev), t.flatten()])[pad:].view(t.shape)
    y2, h2, i2 = off(yd, 1), off(hd, 1), off(idd, 2)
    assert y2.data_ptr() % 16 == 4 and h2.data_ptr() % 16 == 4 and i2.data_ptr() % 8 == 4
    np.testing.assert_array_equal(ec.step_ladder_cost(y2, h2, i2, ladder, dt).cpu().numpy(), want)


def test_kernel_refusals(dev, normal):
    from shallow_ntc_amd import _capi as capi
    from shallow_ntc_amd import entropy_coding as ec
    from shallow_ntc_amd import ops
    _, dt, _ = normal
    lib = capi.load()
    n, hw, c = 2, 5, 8
    y = torch.zeros((n, hw, 1, c), dtype=torch.float32, device=dev)
    ids = torch.zeros((n, hw, 1, c), dtype=torch.int16, device=dev)
    st, inv, sh = ec.step_tensors(list(range(-8, 9)), dev)                  # 17 entries
    cost = torch.zeros((n, 17), dtype=torch.int64, device=dev)
    sym = torch.zeros((n, hw, 1, c), dtype=torch.int32, device=dev)
    out = torch.zeros_like(y)
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = ops._stream()

    def ladder(yp=p(y), mp=p(y), ip=p(ids), vp=p(inv), sp=p(sh), k=5, cc=c, stride=c, mt=p(dt.meta), cq=p(dt.cost_q), cp=p(cost), nt=dt.ntables):
        return lib.sntc_step_ladder_cost(yp, mp, n, hw, cc, stride, ip, vp, sp, k, mt, nt, dt.total, cq, cp, stream)

    def symbols(yp=p(y), mp=p(y), ip=p(ids), vp=p(inv), sp=p(sh), op=p(sym), tp=p(ids), cc=c, stride=c):
        return lib.sntc_step_symbols(yp, mp, n, hw, cc, stride, ip, vp, sp, op, tp, stream)

    def dequant(sp=p(sym), mp=p(y), vp=p(st), op=p(out), cc=c, stride=c):
        return lib.sntc_dequant_step(sp, mp, n, hw, cc, stride, vp, op, stream)

    assert ladder() == capi.OK and symbols() == capi.OK and dequant() == capi.OK
    null = C.c_void_p(0)
    bad = capi.ERR_BAD_SHAPE
    assert ladder(k=0) == bad and ladder(k=17) == bad and ladder(k=16) == capi.OK and ladder(k=1) == capi.OK
    assert ladder(cc=6, stride=6) == bad and symbols(cc=6, stride=6) == bad and dequant(cc=6, stride=6) == bad
    assert ladder(cc=2, stride=4) == bad and ladder(stride=4) == bad and ladder(stride=10) == bad and ladder(nt=63) == bad
    for name in ("yp", "mp", "ip", "vp", "sp", "mt", "cq", "cp"):
        assert ladder(**{name: null}) == bad, name
    for name in ("yp", "mp", "ip", "vp", "sp", "op", "tp"):
        assert symbols(**{name: null}) == bad, name
    for name in ("sp", "mp", "vp", "op"):
        assert dequant(**{name: null}) == bad, name
    assert lib.sntc_step_table_ids(null, n, hw * c, p(sh), p(ids), stream) == bad
    torch.cuda.synchronize()
    assert "sntc_step" in capi.last_error() or "sntc_dequant_step" in capi.last_error()


# ------------------------------------------------------------------ codec --------------------------------------------------
def latents(model, x):
    lat = model.infer_latent_rvs(x)
    return lat.uq[0].loc.contiguous(), lat.uq[1].loc.contiguous()


def sse_of(px, x):
    n = x.shape[0]
    return ((px.cpu().numpy().astype(np.int64) - np.rint((x.cpu().numpy().astype(np.float64) + 0.5) * 255)) ** 2).reshape(n, -1).sum(axis=1)


@pytest.mark.parametrize("n,h,w", [(2, 128, 128), (1, 200, 120)])
def test_step_zero_is_todays_file(n, h, w, dev, hyper_model):
    model = hyper_model
    x = images(n, h, w, dev)
    plain = model.compress(x)
    assert plain[4] == 3
    assert model.compress(x, step=0) == plain
    assert model.compress(x, step=[0] * n) == plain
    z, y = latents(model, x)
    assert model._get_codec().compress_latents(z, y, (h, w), step=0) == plain
    a, b = model.coded_cost(x), model.coded_cost(x, step=0)
    assert all(a[k].tolist() == b[k].tolist() for k in ("bits_z", "bits_y", "sse", "J"))


@pytest.mark.parametrize("n,h,w,steps", [(2, 128, 128, [3, -2]), (1, 200, 120, [7])])
def test_stepped_file(n, h, w, steps, dev, hyper_model):
    from shallow_ntc_amd import entropy_coding as ec
    model = hyper_model
    codec = model._get_codec()
    x = images(n, h, w, dev)
    blob = model.compress(x, step=steps)
    assert blob[:4] == b"SNTC" and blob[4] == 5
    hd = codec._parse(blob)
    assert hd["steps"] == steps and hd["grid"].kind == "image" and hd["grid"].steps == steps
    # decompress = decode of the step symbols at that step; the symbols are the float32 rule on the encoder's y and mu
    z, y = latents(model, x)
    zi, _, sym, ytid, hyper = codec._symbols(z, y, ec.StepGrid.image(steps))
    c = y.shape[-1]
    want_sym, want_tid, _ = np_step_symbols(y.cpu().numpy(), hyper[..., :c].cpu().numpy(), ec.scale_table_ids(hyper).cpu().numpy(), steps)
    np.testing.assert_array_equal(sym.cpu().numpy(), want_sym)
    np.testing.assert_array_equal(ytid.cpu().numpy(), want_tid)
    px = model.decompress(blob)
    assert torch.equal(px, model.decode(ec.int_to_float(zi), sym, (h, w), step=steps))
    assert not torch.equal(px, model.decompress(model.compress(x)))
    # the streams of image i are those of image i compressed alone at its step
    for i in range(n):
        alone = model.compress(x[i:i + 1], step=steps[i])
        assert image_words(model, alone, 0) == image_words(model, blob, i)
        if n > 1:
            assert torch.equal(model.decompress(alone)[0], px[i])
    # the payload against the exact coded cost, the distortion against the decoded pixels
    cost = model.coded_cost(x, step=steps)
    bits, hd = payload_bits(model, blob)
    for i in range(n):
        print(f"\n{n}x{h}x{w} image {i} step {steps[i]}: payload {bits[i]:.0f} bits, cost {cost['bits'][i]:.1f} + flushed {flushed_bits(model, hd):.0f}")
        assert abs(bits[i] - (cost["bits"][i] + flushed_bits(model, hd))) <= slack_bar(model, hd), (i, bits[i], cost["bits"][i])
    assert flushed_bits(model, hd) == codec.flushed_bits(h, w)
    assert cost["sse"].tolist() == sse_of(px, x).tolist()
    if n > 1:
        one = model.coded_cost(x, step=steps[0])
        assert one["bits"][0] == cost["bits"][0] and one["bits"][1] != cost["bits"][1]


def test_ladder_cost_against_latents_cost(dev, hyper_model):
    from shallow_ntc_amd import entropy_coding as ec
    model = hyper_model
    codec = model._get_codec()
    for n, h, w in ((2, 128, 128), (1, 200, 120)):
        x = images(n, h, w, dev)
        z, y = latents(model, x)
        ks = [-32, -16, -5, 0, 7, 16, 32]
        cost_z, cost_y = codec.ladder_cost(z, y, (h, w), ks)
        assert cost_y.dtype == torch.int64 and tuple(cost_y.shape) == (n, len(ks)) and tuple(cost_z.shape) == (n,)
        cost_y = cost_y.cpu().numpy()
        for j, k in enumerate(ks):
            cz, cy, _, _ = codec.latents_cost(z, y, x, step=k)
            assert cy.cpu().numpy().tolist() == cost_y[:, j].tolist(), k
            assert torch.equal(cz, cost_z)
        elems = y[0].numel()
        for i in range(n):
            per = {k: cost_y[i, j] / 65536.0 / elems for j, k in enumerate(ks)}
            print(f"\n{n}x{h}x{w} image {i}: bit / symbol at k = -16, 0, +16: {per[-16]:.3f} {per[0]:.3f} {per[16]:.3f}")
            assert per[16] < per[0] < per[-16]              # steps a factor 7.2 apart (CPU emulation: 0.71 / 2.50 / 5.18 bit per symbol)


def test_target_bpp(dev, hyper_model):
    from shallow_ntc_amd import entropy_coding as ec
    model = hyper_model
    codec = model._get_codec()
    n, h, w = 2, 128, 128
    x = images(n, h, w, dev)
    z, y = latents(model, x)
    ladder = list(range(ec.STEP_MIN, ec.STEP_MAX + 1))
    cost_z, cost_y = codec.ladder_cost(z, y, (h, w), ladder)
    bits = (cost_z.cpu().numpy()[:, None] + cost_y.cpu().numpy()) / 65536.0 + codec.flushed_bits(h, w)       # bits_i(k)
    at = lambda i, k: float(bits[i, ladder.index(k)])

    def between(i, k):
        assert at(i, k) < at(i, k - 1)
        return 0.5 * (at(i, k) + at(i, k - 1)) / (h * w)

    for kstar in (-9, -2, 3):           # the cost of these latents falls strictly down to k ~ 9 (beyond, every symbol is 0)
        # one target for the batch (image 0's), then per-image targets that choose independently
        for targets in (between(0, kstar), [between(0, kstar), between(1, kstar + 5)]):
            blob = model.compress(x, target_bpp=targets)
            rep = model.last_compress_report
            budgets = ec.check_budgets(targets, n) * h * w
            want = [min(k for k in ladder if at(i, k) <= budgets[i]) for i in range(n)]          # the rule, restated
            assert want[0] == kstar and (np.ndim(targets) == 0 or want[1] == kstar + 5)
            pay, hd = payload_bits(model, blob)
            for i in range(n):
                print(f"\ntarget {budgets[i] / (h * w):.4f} bpp image {i}: step {rep[i]['step_chosen']}, predicted {rep[i]['bits_predicted']:.1f}, "
                      f"payload {pay[i]:.0f}, budget {budgets[i]:.1f} bits")
                assert rep[i]["step_chosen"] == want[i] and rep[i]["met"] is True
                assert rep[i]["bits_predicted"] == at(i, want[i]) and rep[i]["budget_bits"] == budgets[i]
                assert pay[i] <= budgets[i] + slack_bar(model, hd)
            assert codec._parse(blob)["steps"] == (want if any(want) else None)
            assert blob == model.compress(x, step=want)
    # a budget nothing meets: the coarsest step, reported as not met, and the file still decodes
    blob = model.compress(x, target_bpp=0.5 * float(bits[:, -1].min()) / (h * w))
    rep = model.last_compress_report
    assert [r["step_chosen"] for r in rep] == [ec.STEP_MAX] * n and not any(r["met"] for r in rep)
    assert [r["bits_predicted"] for r in rep] == bits[:, -1].tolist()
    px = model.decompress(blob)
    assert tuple(px.shape) == (n, h, w, 3) and torch.equal(px, model.decompress(model.compress(x, step=ec.STEP_MAX)))
    # a generous budget: the finest step of the ladder
    model.compress(x, target_bpp=2.0 * float(bits[:, 0].max()) / (h * w))
    assert [r["step_chosen"] for r in model.last_compress_report] == [ec.STEP_MIN] * n


def test_decompress_many_mixes_versions(dev, hyper_model):
    model = hyper_model
    xa, xb = images(2, 128, 128, dev), images(1, 200, 120, dev, seed=4)
    blobs = [model.compress(xa), model.compress(xb, step=[6]), model.compress(xa, step=[-3, 11])]
    assert [b[4] for b in blobs] == [3, 5, 5]
    many = model.decompress_many(blobs)
    for got, blob in zip(many, blobs):
        assert torch.equal(got, model.decompress(blob))


def test_refusals(dev, hyper_model, fact_model, monkeypatch):
    from shallow_ntc_amd import _capi as capi
    from shallow_ntc_amd.mshyper import configs
    from shallow_ntc_amd.mshyper.models import Model
    from test_hip_sga import TC
    model = hyper_model
    x = images(2, 64, 64, dev)
    blob = model.compress(x, step=[1, 2])
    with pytest.raises(capi.SntcError) as e:                    # a factorized model reads v4 only
        fact_model.decompress(blob)
    assert e.value.code == capi.ERR_UNSUPPORTED
    launches = []
    for m in (model, fact_model):
        analysis = m.infer_latent_rvs
        monkeypatch.setattr(m, "infer_latent_rvs", lambda *a, _f=analysis, **k: launches.append(1) or _f(*a, **k))
    with pytest.raises(ValueError, match="exclude"):
        model.compress(x, step=1, target_bpp=0.3)
    with pytest.raises(ValueError, match="itinf"):
        model.compress(x, itinf=dict(steps=2), step=1)
    with pytest.raises(ValueError, match="itinf"):
        model.compress(x, itinf=dict(steps=2), target_bpp=0.3)
    for bad in (33, -33, [1, 33], [1], [1, 2, 3], 1.5, [1, 2.0]):
        with pytest.raises(ValueError):
            model.compress(x, step=bad)
        with pytest.raises(ValueError):
            model.coded_cost(x, step=bad)
    for bad in ([0.3], [0.1, 0.2, 0.3], float("inf")):
        with pytest.raises(ValueError):
            model.compress(x, target_bpp=bad)
    for kw in (dict(step=1), dict(step=0), dict(target_bpp=0.3)):
        with pytest.raises(NotImplementedError, match="factorized"):
            fact_model.compress(x, **kw)
    with pytest.raises(NotImplementedError, match="factorized"):
        fact_model.coded_cost(x, step=1)
    with pytest.raises(NotImplementedError, match="factorized"):
        fact_model.decode(torch.zeros((1, 4, 4, 8), device=dev), None, (64, 64), step=1)
    split = Model(device=dev, rd_lambda=0.02, transform_config=TC, precision="bf16x3")
    monkeypatch.setattr(split, "infer_latent_rvs", lambda *a, **k: launches.append(1))
    for kw in (dict(step=1), dict(target_bpp=0.3)):
        with pytest.raises(NotImplementedError, match="bf16x3"):
            split.compress(x, **kw)
    with pytest.raises(NotImplementedError, match="bf16x3"):
        split.coded_cost(x, step=2)
    assert not launches                                         # every refusal came before the analysis ran
