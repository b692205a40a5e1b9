"""Region-of-interest coding (-m gpu; DESIGN.md 4.7, "variable rate"): the per-position quantisation-step kernels of
csrc/quant_step.hip against their NumPy restatement (integer / bit equality) and against the per-image instances of the same
kernels, the map ladder cost against ``np_cost``, wire format v7 through compress / decompress, rate control over a map
and the refusals."""
from fractions import Fraction

import ctypes as C
import numpy as np
import pytest
import torch

from test_hip_itinf_bitstream import (big_table_set, fact_model, flushed_bits, hyper_model, image_words, images,  # noqa: F401
                                      payload_bits, slack_bar)
from test_hip_quant_step import (LADDERS, N, STEPS, STRIDE_CASES, case_of, dev_case, dv, latents, normal, offset_view,  # noqa: F401
                                 round_f32, sse_of)
from test_rans_cost_host import np_cost, ref_cost_table

pytestmark = pytest.mark.gpu

# N = 3 images; positions per image around a wave, one workgroup pass (256 threads x 4 channels at c = 4) and many workgroups; at
# c = 320 the position counts of the same neighbourhoods of test_hip_quant_step.CASES.  mu rows of c and of 2 c floats.
CASES = [(hw * 4, 4, s) for hw in (1, 15, 16, 17, 255, 256, 257, 1025) for s in (4, 8)] + \
        [(hw * 320, 320, s) for hw in (1, 3, 13, 219) for s in (320, 640)]
IDS = [f"hw{E // c}-c{c}-stride{s}" for E, c, s in CASES]
MAPS = ("mod3", "random", "halves")


def pinned(E, c, hw):
    """The positions of make_case's tie elements (the first 8 of an image) and escape elements (its last 6): they were built for
    the image's STEPS entry and keep it in every map."""
    first, last = np.arange(0, min(8, E)) // c, np.arange(max(E - 6, 0), E) // c
    return np.unique(np.concatenate([first, last]))


def make_map(kind, cs, lo=-32, hi=32, pin=True):
    """int8 [N, hw]: (a) p mod 3 -> (lo, 0, hi), (b) seeded random in [lo, hi], (c) two halves split at hw // 2."""
    hw = cs["hw"]
    p = np.arange(hw)
    if kind == "mod3":
        K = np.broadcast_to(np.array([lo, 0, hi])[p % 3], (N, hw)).copy()
    elif kind == "random":
        K = np.random.default_rng(cs["E"] + cs["c"]).integers(lo, hi + 1, size=(N, hw))
    else:
        K = np.stack([np.where(p < hw // 2, a, b) for a, b in ((lo, hi), (hi, 7), (-5, lo))])
    if pin:
        K[:, pinned(cs["E"], cs["c"], hw)] = np.array(STEPS)[:, None]
    return K.astype(np.int8)


def np_map_symbols(y, mu, ids, K):
    """The rule in float32 NumPy at one ladder index per position (K [N, hw], shared by the position's channels):
    s = rint((y - mu) * inv_step(K)) (a float32 subtract, then a float32 multiply; half to even), t = clip(t0 - K, 0, 63)."""
    from shallow_ntc_amd import entropy_coding as ec
    lut = np.array([ec.step_size(-k) for k in range(ec.STEP_MIN, ec.STEP_MAX + 1)], np.float32)
    K = np.asarray(K, np.int64)[..., None]
    d = (y.astype(np.float32) - mu.astype(np.float32)).astype(np.float32)
    p = (d * lut[K - ec.STEP_MIN]).astype(np.float32)
    return np.rint(p).astype(np.int32), np.clip(ids.astype(np.int64) - K, 0, 63).astype(np.int16), p


def dmap(K, dev):
    """[N, hw] -> int8 [N, hw, 1] on the device (NHWC latents with w = 1)."""
    return dv(np.asarray(K, np.int8), dev).unsqueeze(2)


@pytest.fixture(scope="module")
def lut(dev):
    from shallow_ntc_amd import entropy_coding as ec
    t = ec.step_lut(dev)
    host = t.cpu().numpy()
    assert host.shape == (2, 65) and host.dtype == np.float32
    assert host[0].tolist() == [ec.step_size(k) for k in range(-32, 33)] and host[1].tolist() == [ec.step_size(-k) for k in range(-32, 33)]
    return t


# ------------------------------------------------------------------ kernels ------------------------------------------------
@pytest.mark.parametrize("E,c,stride", CASES, ids=IDS)
def test_map_kernels_are_the_float32_rule(E, c, stride, dev, lut):
    from shallow_ntc_amd import entropy_coding as ec
    from shallow_ntc_amd import ops
    cs = case_of(E, c, stride)
    y, hyper, ids = dev_case(cs, dev)
    rng = np.random.default_rng(E + stride)
    seen_ties = np.zeros(N, bool)
    for kind in MAPS:
        K = make_map(kind, cs)
        want_sym, want_tid, scaled = np_map_symbols(cs["y"], cs["mu"], cs["ids"], K)
        kd = dmap(K, dev)
        sym, tid = ops.step_map_symbols(y, hyper, ids, kd, lut)
        np.testing.assert_array_equal(sym.cpu().numpy().reshape(want_sym.shape), want_sym)
        np.testing.assert_array_equal(tid.cpu().numpy().reshape(want_tid.shape), want_tid)
        np.testing.assert_array_equal(ec.step_map_table_ids(ids, kd).cpu().numpy().reshape(want_tid.shape), want_tid)
        # the inputs still exercise what make_case built: escapes on both sides, exact ties in every image
        assert (want_sym > 4096).any() and (want_sym < -4096).any()
        frac = scaled - np.floor(scaled)
        seen_ties |= (frac == 0.5).reshape(N, -1).any(axis=1)
        # values: the correctly rounded float32 of the exact mu + step(K) * s (ONE rounding) on a sample; everywhere the value
        # sntc_dequant_step gives at that index
        got = ops.dequant_step_map(dv(want_sym, dev).unsqueeze(2), hyper, kd, lut).cpu().numpy().reshape(N, -1)
        s_flat, mu_flat, k_flat = want_sym.reshape(N, -1), np.ascontiguousarray(cs["mu"]).reshape(N, -1), np.repeat(K, c, axis=1)
        pick = np.unique(np.concatenate([np.arange(min(E, 40)), np.arange(max(E - 20, 0), E), rng.integers(0, E, 60)]))
        for b in range(N):
            want = np.array([round_f32(Fraction(float(mu_flat[b, j])) + Fraction(ec.step_size(int(k_flat[b, j]))) * int(s_flat[b, j]))
                             for j in pick], np.float32)
            np.testing.assert_array_equal(got[b, pick].view(np.uint32), want.view(np.uint32))
        whole = np.empty_like(got)
        for k in np.unique(K):
            at = ops.dequant_step(dv(want_sym, dev).unsqueeze(2), hyper, ec.step_tensors([int(k)] * N, dev)[0]).cpu().numpy().reshape(N, -1)
            whole[k_flat == k] = at[k_flat == k]
        np.testing.assert_array_equal(got.view(np.uint32), whole.view(np.uint32))
    assert seen_ties.all()
    # both ends of the table ladder are clamped to: position 0 of every image holds ids 0 and 63
    assert (cs["ids"][0].astype(int) + 32 > 63).any() and (cs["ids"][2].astype(int) - 32 < 0).any()


@pytest.mark.parametrize("E,c,stride", CASES, ids=IDS)
def test_uniform_map_is_the_per_image_kernels(E, c, stride, dev, lut, normal):
    """A map that is constant per image, at STEPS = [-32, 5, 32]: the symbols, ids, values and ladder costs of sntc_step_symbols,
    sntc_step_table_ids, sntc_dequant_step and sntc_step_ladder_cost, bit for bit."""
    from shallow_ntc_amd import entropy_coding as ec
    from shallow_ntc_amd import ops
    _, dt, _ = normal
    cs = case_of(E, c, stride)
    y, hyper, ids = dev_case(cs, dev)
    kd = dmap(np.broadcast_to(np.array(STEPS)[:, None], (N, cs["hw"])), dev)
    st, inv, sh = ec.step_tensors(STEPS, dev)
    sym0, tid0 = ops.step_symbols(y, hyper, ids, inv, sh)
    sym, tid = ops.step_map_symbols(y, hyper, ids, kd, lut)
    assert torch.equal(sym, sym0) and torch.equal(tid, tid0)
    assert torch.equal(ec.step_map_table_ids(ids, kd), ec.step_table_ids(ids, sh))
    assert torch.equal(ops.dequant_step_map(sym, hyper, kd, lut).view(torch.int32), ops.dequant_step(sym0, hyper, st).view(torch.int32))
    # ladder: with offsets 0 candidate j is the uniform step j; with a constant offset o per image it is the step j + o
    zero = dmap(np.zeros((N, cs["hw"])), dev)
    for ladder in LADDERS:
        assert torch.equal(ec.step_map_ladder_cost(y, hyper, ids, zero, ladder, dt, lut), ec.step_ladder_cost(y, hyper, ids, ladder, dt))
    shifted = ec.step_map_ladder_cost(y, hyper, ids, kd, [-4, 0, 3], dt, lut).cpu().numpy()
    for b, k in enumerate(STEPS):
        want = ec.step_ladder_cost(y, hyper, ids, [int(np.clip(k + j, -32, 32)) for j in (-4, 0, 3)], dt).cpu().numpy()
        assert shifted[b].tolist() == want[b].tolist()


BASES = [[-32], [32], [-32, -7, 0, 9, 32], [-32, -20, -11, -5, -3, -2, -1, 0, 1, 2, 3, 6, 12, 19, 27, 32]]


def np_ladder(y, mu, ids, offsets, bases, tabs, q):
    """np_cost of the NumPy symbols at clip(base + offsets), one column per base -> int64 [n, len(bases)]."""
    n = y.shape[0]
    cols = []
    for b in bases:
        sym, tid, _ = np_map_symbols(y, mu, ids, np.clip(int(b) + offsets.astype(np.int64), -32, 32))
        cols.append(np_cost(sym.reshape(n, -1), tid.reshape(n, -1), tabs, q))
    return np.stack(cols, axis=1)


@pytest.mark.parametrize("E,c,stride", CASES, ids=IDS)
def test_map_ladder_cost_is_the_numpy_sum(E, c, stride, dev, lut, normal):
    """Every [image, candidate] entry = np_cost of the NumPy symbols at clip(base + offsets), for 1, 5 and 16 candidates, with
    offsets in [-64, 64] that push the index past both ends of the ladder."""
    from shallow_ntc_amd import entropy_coding as ec
    tabs, dt, q = normal
    cs = case_of(E, c, stride)
    y, hyper, ids = dev_case(cs, dev)
    for kind in MAPS:
        off = make_map(kind, cs, -64, 64, pin=False)
        assert kind != "mod3" or cs["hw"] < 3 or ((off + 32 > 32).any() and (off - 32 < -32).any())    # past both ends at any base
        od = dmap(off, dev)
        for bases in BASES:
            got = ec.step_map_ladder_cost(y, hyper, ids, od, bases, dt, lut)
            assert got.dtype == torch.int64 and tuple(got.shape) == (N, len(bases))
            np.testing.assert_array_equal(got.cpu().numpy(), np_ladder(cs["y"], cs["mu"], cs["ids"], off, bases, tabs, q))
    # more candidates than one launch takes: chunks of 16
    whole = list(range(ec.STEP_MIN, ec.STEP_MAX + 1, 3)) + [0]
    got = ec.step_map_ladder_cost(y, hyper, ids, od, whole, dt, lut).cpu().numpy()
    np.testing.assert_array_equal(got, np_ladder(cs["y"], cs["mu"], cs["ids"], off, whole, tabs, q))


def test_map_ladder_cost_with_tables_beyond_the_lds_limit(dev, lut):
    """Descriptors and costs read from global memory (84 tables; the ladder is their first 64): the same exact sums, from
    aligned tensors and from views 4 bytes into their allocation (the element-wise load path; the map 1 byte into its own)."""
    from shallow_ntc_amd import entropy_coding as ec
    big = big_table_set()
    db, q = ec.DeviceTables(big, dev), ref_cost_table(big)
    for key in ((4100, 4, 8), (70080, 320, 320)):
        cs = case_of(*key)
        y, hyper, ids = dev_case(cs, dev)
        off = make_map("random", cs, -64, 64, pin=False)
        od = dmap(off, dev)
        want = np_ladder(cs["y"], cs["mu"], cs["ids"], off, BASES[2], big, q)
        np.testing.assert_array_equal(ec.step_map_ladder_cost(y, hyper, ids, od, BASES[2], db, lut).cpu().numpy(), want)
        y2, h2, i2, o2 = offset_view(y, 1, dev), offset_view(hyper, 1, dev), offset_view(ids, 2, dev), offset_view(od, 1, dev)
        assert y2.data_ptr() % 16 == 4 and h2.data_ptr() % 16 == 4 and i2.data_ptr() % 8 == 4 and o2.data_ptr() % 2 == 1
        np.testing.assert_array_equal(ec.step_map_ladder_cost(y2, h2, i2, o2, BASES[2], db, lut).cpu().numpy(), want)


def test_map_ladder_cost_from_an_offset_view(dev, lut, normal):
    """y, mu and the ids each start 4 bytes into their allocation (the map 1 byte into its own): the element-wise load path
    (V = 1) on sizes that would take the vector path, the same sums."""
    from shallow_ntc_amd import entropy_coding as ec
    tabs, dt, q = normal
    for key in ((4100, 4, 4), (4160, 320, 640)):
        cs = case_of(*key)
        y, hyper, ids = dev_case(cs, dev)
        off = make_map("random", cs, -64, 64, pin=False)
        od = dmap(off, dev)
        want = np_ladder(cs["y"], cs["mu"], cs["ids"], off, BASES[3], tabs, q)
        y2, h2, i2, o2 = offset_view(y, 1, dev), offset_view(hyper, 1, dev), offset_view(ids, 2, dev), offset_view(od, 1, dev)
        assert y2.data_ptr() % 16 == 4 and h2.data_ptr() % 16 == 4 and i2.data_ptr() % 8 == 4 and o2.data_ptr() % 2 == 1
        for a, b, cc, oo in ((y, hyper, ids, od), (y2, h2, i2, o2), (y2, hyper, ids, od), (y, h2, ids, od), (y, hyper, i2, od), (y, hyper, ids, o2)):
            np.testing.assert_array_equal(ec.step_map_ladder_cost(a, b, cc, oo, BASES[3], dt, lut).cpu().numpy(), want)


@pytest.mark.parametrize("n,hw,c,stride", STRIDE_CASES, ids=[f"n{n}-hw{hw}-c{c}-stride{s}" for n, hw, c, s in STRIDE_CASES])
def test_map_ladder_cost_over_several_passes(n, hw, c, stride, dev, lut, normal):
    """The grid-stride advance (position, unit in the position) with an offset per position, on both load paths: units per image
    exceed what the launch's workgroups take in one pass by a non-multiple (test_hip_quant_step.STRIDE_CASES)."""
    from shallow_ntc_amd import entropy_coding as ec
    tabs, dt, q = normal
    for per_unit in (4, 1):
        units = hw * c // per_unit
        grid = min(-(-units // 1024), max(1, 512 // n))
        assert units > grid * 1024 and units % (grid * 1024) != 0
    rng = np.random.default_rng(n + hw + c + stride)
    ids = rng.integers(0, 64, size=(n, hw, c)).astype(np.int16)
    rows = (rng.standard_normal((n, hw, stride)) * 2.0).astype(np.float32)
    sig = 0.11 * np.exp(ec.SCALE_FACTOR * ids.astype(np.float64))
    y = (rows[..., :c] + rng.standard_normal((n, hw, c)) * sig * np.where(rng.random((n, hw, c)) < 0.2, 3.5, 1.0)).astype(np.float32)
    y.reshape(n, -1)[:, -4:] += np.array([20000.0, -20000.0, 300.0, -300.0], np.float32)         # escapes in the last pass
    off = rng.integers(-40, 41, size=(n, hw)).astype(np.int8)
    off[:, -1] = 0
    yd, hd, idd = (dv(a, dev).unsqueeze(2) for a in (y, rows, ids))
    od = dmap(off, dev)
    bases = [-32, 0, 5]
    want = np_ladder(y, rows[..., :c], ids, off, bases, tabs, q)
    np.testing.assert_array_equal(ec.step_map_ladder_cost(yd, hd, idd, od, bases, dt, lut).cpu().numpy(), want)
    y2, h2, i2 = offset_view(yd, 1, dev), offset_view(hd, 1, dev), offset_view(idd, 2, dev)
    np.testing.assert_array_equal(ec.step_map_ladder_cost(y2, h2, i2, od, bases, dt, lut).cpu().numpy(), want)


def test_kernel_refusals(dev, lut, normal):
    from shallow_ntc_amd import _capi as capi
    from shallow_ntc_amd import ops
    _, dt, _ = normal
    lib = capi.load()
    n, hw, c = 2, 5, 8
    y = torch.zeros((n, hw, 1, c), dtype=torch.float32, device=dev)
    ids = torch.zeros((n, hw, 1, c), dtype=torch.int16, device=dev)
    kmap = torch.zeros((n, hw, 1), dtype=torch.int8, device=dev)
    base = torch.arange(-8, 9, dtype=torch.int32, device=dev)              # 17 entries
    cost = torch.zeros((n, 17), dtype=torch.int64, device=dev)
    sym = torch.zeros((n, hw, 1, c), dtype=torch.int32, device=dev)
    out = torch.zeros_like(y)
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = ops._stream()

    def ladder(yp=p(y), mp=p(y), ip=p(ids), op=p(kmap), lp=p(lut), bp=p(base), k=5, cc=c, stride=c, mt=p(dt.meta), cq=p(dt.cost_q), cp=p(cost),
               nt=dt.ntables, nn=n):
        return lib.sntc_step_map_ladder_cost(yp, mp, nn, hw, cc, stride, ip, op, lp, bp, k, mt, nt, dt.total, cq, cp, stream)

    def symbols(yp=p(y), mp=p(y), ip=p(ids), kp=p(kmap), lp=p(lut), op=p(sym), tp=p(ids), cc=c, stride=c, nn=n):
        return lib.sntc_step_map_symbols(yp, mp, nn, hw, cc, stride, ip, kp, lp, op, tp, stream)

    def dequant(sp=p(sym), mp=p(y), kp=p(kmap), lp=p(lut), op=p(out), cc=c, stride=c, nn=n):
        return lib.sntc_dequant_step_map(sp, mp, nn, hw, cc, stride, kp, lp, op, stream)

    def table_ids(ip=p(ids), kp=p(kmap), tp=p(ids), nn=n, cc=c, pos=hw):
        return lib.sntc_step_map_table_ids(ip, nn, pos, cc, kp, tp, stream)

    assert ladder() == capi.OK and symbols() == capi.OK and dequant() == capi.OK and table_ids() == capi.OK
    null = C.c_void_p(0)
    bad = capi.ERR_BAD_SHAPE
    assert ladder(k=0) == bad and ladder(k=17) == bad and ladder(k=16) == capi.OK and ladder(k=1) == capi.OK
    assert ladder(cc=6, stride=6) == bad and symbols(cc=6, stride=6) == bad and dequant(cc=6, stride=6) == bad
    assert ladder(cc=2, stride=4) == bad and ladder(stride=4) == bad and ladder(stride=10) == bad and ladder(nt=63) == bad
    assert ladder(nn=0) == bad and symbols(nn=0) == bad and dequant(nn=65536) == bad and table_ids(nn=0) == bad
    assert table_ids(cc=0) == bad and table_ids(pos=0) == bad
    for name in ("yp", "mp", "ip", "op", "lp", "bp", "mt", "cq", "cp"):
        assert ladder(**{name: null}) == bad, name
    for name in ("yp", "mp", "ip", "kp", "lp", "op", "tp"):
        assert symbols(**{name: null}) == bad, name
    for name in ("sp", "mp", "kp", "lp", "op"):
        assert dequant(**{name: null}) == bad, name
    for name in ("ip", "kp", "tp"):
        assert table_ids(**{name: null}) == bad, name
    room = torch.zeros((n * hw * c + 4,), dtype=torch.float32, device=dev)
    odd = C.c_void_p(room.data_ptr() + 4)                               # 4 bytes in: fine for the ladder, refused by the vector kernels
    assert ladder(yp=odd) == capi.OK and symbols(yp=odd) == bad and dequant(mp=odd) == bad and symbols(tp=C.c_void_p(ids.data_ptr() + 4)) == bad
    torch.cuda.synchronize()
    assert "sntc_step_map" in capi.last_error() or "sntc_dequant_step_map" in capi.last_error()
    # the wrappers refuse a map or a table of the wrong shape / dtype before the call
    for km, lt in ((kmap[:, :4], lut), (kmap.to(torch.int32), lut), (kmap.cpu(), lut), (kmap, lut[:, :64]), (kmap, lut.double())):
        with pytest.raises(ValueError):
            ops.step_map_symbols(y, y, ids, km, lt)
        with pytest.raises(ValueError):
            ops.dequant_step_map(sym, y, km, lt)


# ------------------------------------------------------------------ codec --------------------------------------------------
def offsets_for(model, n, h, w, seed=0):
    """Offsets that vary inside every image: blocks of a few positions, values over [-40, 40], the corners pinned to 0, 40, -40
    (past both ends of the ladder at the steps the tests use) and 17."""
    hh, ww = model.step_offsets_shape(h, w)
    rng = np.random.default_rng(seed + h + w)
    coarse = rng.integers(-40, 41, size=(n, -(-hh // 3), -(-ww // 2)))
    off = np.repeat(np.repeat(coarse, 3, axis=1), 2, axis=2)[:, :hh, :ww].astype(np.int8)
    off[:, 0, 0], off[:, 0, -1], off[:, -1, 0], off[:, -1, -1] = 0, 40, -40, 17
    return off


@pytest.mark.parametrize("n,h,w", [(2, 128, 128), (1, 200, 120)])
def test_constant_offsets_are_todays_files(n, h, w, dev, hyper_model):
    model = hyper_model
    x = images(n, h, w, dev)
    hh, ww = model.step_offsets_shape(h, w)
    assert (hh, ww) == tuple(latents(model, x)[1].shape[1:3])
    zero = np.zeros((n, hh, ww), np.int8)
    plain = model.compress(x)
    assert plain[4] == 3
    assert model.compress(x, step_offsets=zero) == plain
    assert model.compress(x, step=0, step_offsets=zero.astype(np.int64)) == plain
    assert model.compress(x, step_offsets=torch.from_numpy(zero)) == plain
    steps = [3, -2][:n]
    stepped = model.compress(x, step=steps)
    assert stepped[4] == 5
    assert model.compress(x, step=steps, step_offsets=zero) == stepped
    assert model.compress(x, step_offsets=zero + np.array(steps, np.int8).reshape(n, 1, 1)) == stepped
    assert model.compress(x, step=1, step_offsets=zero + np.array(steps, np.int8).reshape(n, 1, 1) - 1) == stepped
    assert model.compress(x, step=30, step_offsets=zero + 64) == model.compress(x, step=32)          # clipped to the ladder's end
    z, y = latents(model, x)
    assert model._get_codec().compress_latents(z, y, (h, w), step_offsets=zero) == plain
    a, b = model.coded_cost(x, step=steps), model.coded_cost(x, step_offsets=zero + np.array(steps, np.int8).reshape(n, 1, 1))
    assert all(a[k].tolist() == b[k].tolist() for k in ("bits_z", "bits_y", "sse", "J"))


@pytest.mark.parametrize("n,h,w,steps", [(2, 128, 128, [3, -2]), (1, 200, 120, [7])])
def test_mapped_file(n, h, w, steps, dev, hyper_model):
    from shallow_ntc_amd import entropy_coding as ec
    model = hyper_model
    codec = model._get_codec()
    x = images(n, h, w, dev)
    off = offsets_for(model, n, h, w)
    K = np.clip(np.array(steps).reshape(n, 1, 1) + off.astype(np.int64), -32, 32)
    assert (K == 32).any() and (K == -32).any() and (np.array(steps).reshape(n, 1, 1) + off > 32).any()      # clipped at both ends
    blob = model.compress(x, step=steps, step_offsets=off)
    assert blob[:4] == b"SNTC" and blob[4] == 7
    hd = codec._parse(blob)
    assert hd["steps"] is None and hd["kmap"].dtype == np.int8 and (hd["kmap"] == K).all()
    assert hd["grid"].kind == "map" and hd["grid"].kmap is hd["kmap"]
    # the symbols are the float32 rule on the encoder's y and mu; decompress = decode of them with the same offsets
    z, y = latents(model, x)
    zi, _, sym, ytid, hyper = codec._symbols(z, y, ec.StepGrid("map", n, kmap=K.astype(np.int8)))
    c = y.shape[-1]
    flat = lambda t: t.cpu().numpy().reshape(n, -1, t.shape[-1])
    want_sym, want_tid, _ = np_map_symbols(flat(y), flat(hyper[..., :c]), flat(ec.scale_table_ids(hyper)), K.reshape(n, -1))
    np.testing.assert_array_equal(flat(sym), want_sym)
    np.testing.assert_array_equal(flat(ytid), want_tid)
    px = model.decompress(blob)
    assert torch.equal(px, model.decode(ec.int_to_float(zi), sym, (h, w), step=steps, step_offsets=off))
    assert not torch.equal(px, model.decompress(model.compress(x, step=steps)))
    # the streams of image i are those of image i compressed alone with its own map
    for i in range(n):
        alone = model.compress(x[i:i + 1], step=steps[i], step_offsets=off[i:i + 1])
        assert alone[4] == 7 and image_words(model, alone, 0) == image_words(model, blob, i)
        if n > 1:
            assert torch.equal(model.decompress(alone)[0], px[i])
    # the payload against the exact coded cost, the distortion against the decoded pixels
    cost = model.coded_cost(x, step=steps, step_offsets=off)
    bits, hd = payload_bits(model, blob)
    for i in range(n):
        print(f"\n{n}x{h}x{w} image {i} step {steps[i]} + offsets: payload {bits[i]:.0f} bits, cost {cost['bits'][i]:.1f} + flushed {flushed_bits(model, hd):.0f}")
        assert abs(bits[i] - (cost["bits"][i] + flushed_bits(model, hd))) <= slack_bar(model, hd), (i, bits[i], cost["bits"][i])
    assert cost["sse"].tolist() == sse_of(px, x).tolist()
    # the ladder over the map: candidate j = latents_cost at step j with these offsets
    ks = [-32, -5, 0, 7, 32]
    cost_z, cost_y = codec.ladder_cost(z, y, (h, w), ks, step_offsets=off)
    for j, k in enumerate(ks):
        cz, cy, _, _ = codec.latents_cost(z, y, x, step=k, step_offsets=off)
        assert cy.cpu().numpy().tolist() == cost_y[:, j].cpu().numpy().tolist() and torch.equal(cz, cost_z), k


def test_decompress_many_mixes_versions(dev, hyper_model):
    model = hyper_model
    xa, xb = images(2, 128, 128, dev), images(1, 200, 120, dev, seed=4)
    blobs = [model.compress(xa), model.compress(xb, step=[6]), model.compress(xa, step=[-3, 11], step_offsets=offsets_for(model, 2, 128, 128)),
             model.compress(xb, step_offsets=offsets_for(model, 1, 200, 120, seed=5))]
    assert [b[4] for b in blobs] == [3, 5, 7, 7]
    many = model.decompress_many(blobs)
    for got, blob in zip(many, blobs):
        assert torch.equal(got, model.decompress(blob))


def test_it_is_roi_coding(dev, hyper_model):
    """Offsets 0 on a rectangle, +16 around it: fewer bits than the uniform step-0 file, the same pixels well inside the
    rectangle, other pixels outside.
    Margin: the synthesis is a 13 x 13 stride-8 transposed convolution (base and residual read the same input; the activation
    between is per position) and a 5 x 5 stride-2 one.  A pixel reads hidden positions at most (5 - 1) / 2 / 2 = 1, + 1 for the
    alignment of the strided grid, = 2 away from its own; a hidden position reads latents whose 8-spaced footprint centre is at
    most (13 - 1) / 2 = 6, + 7 for the alignment, away: 2 + 6 + 7 = 15 hidden positions < 16 = 2 latent positions.  So a pixel
    whose latent position lies 2 or more inside the rectangle on every side reads no latent outside it."""
    model = hyper_model
    margin = -(-(2 + 6 + 7) // 8)
    assert margin == 2
    H = W = 256
    x = images(1, H, W, dev)
    hh, ww = model.step_offsets_shape(H, W)
    assert (hh, ww) == (16, 16)
    r0, r1, c0, c1 = 3, 12, 4, 14                        # the rectangle, in latent positions [r0, r1) x [c0, c1)
    off = np.full((1, hh, ww), 16, np.int8)
    off[:, r0:r1, c0:c1] = 0
    uniform, roi = model.compress(x, step=0), model.compress(x, step_offsets=off)
    assert uniform[4] == 3 and roi[4] == 7
    cu, cr = model.coded_cost(x, step=0), model.coded_cost(x, step_offsets=off)
    print(f"\nbits_y uniform {cu['bits_y'][0]:.0f}, ROI {cr['bits_y'][0]:.0f}; file {len(uniform)} -> {len(roi)} bytes")
    assert cr["bits_y"][0] < cu["bits_y"][0] and cr["bits_z"][0] == cu["bits_z"][0]
    pu, pr = model.decompress(uniform)[0].cpu().numpy(), model.decompress(roi)[0].cpu().numpy()
    f = 16
    inner = (slice((r0 + margin) * f, (r1 - margin) * f), slice((c0 + margin) * f, (c1 - margin) * f))
    assert pu[inner].size >= 64 * 64 * 3
    np.testing.assert_array_equal(pr[inner], pu[inner])
    outside = np.ones((H, W), bool)
    outside[r0 * f:r1 * f, c0 * f:c1 * f] = False
    differ = (pr != pu).any(axis=-1)
    print(f"pixels that differ: {differ[outside].mean():.3f} of the outside, {differ[~outside].mean():.3f} of the rectangle")
    for band in (differ[:r0 * f], differ[r1 * f:], differ[:, :c0 * f], differ[:, c1 * f:]):      # on every side of the rectangle
        assert band.any()


def test_target_bpp_with_offsets(dev, hyper_model):
    from shallow_ntc_amd import entropy_coding as ec
    model = hyper_model
    codec = model._get_codec()
    n, h, w = 2, 128, 128
    x = images(n, h, w, dev)
    off = offsets_for(model, n, h, w)
    off = np.clip(off, -12, 12).astype(np.int8)
    z, y = latents(model, x)
    ladder = list(range(ec.STEP_MIN, ec.STEP_MAX + 1))
    cost_z, cost_y = codec.ladder_cost(z, y, (h, w), ladder, step_offsets=off)
    map_bits = 24.0 * ec.count_runs(off)
    assert (map_bits > 24).all()
    bits = (cost_z.cpu().numpy()[:, None] + cost_y.cpu().numpy()) / 65536.0 + codec.flushed_bits(h, w) + map_bits[:, None]
    at = lambda i, k: float(bits[i, ladder.index(k)])

    def between(i, k):
        assert at(i, k) < at(i, k - 1)
        return 0.5 * (at(i, k) + at(i, k - 1)) / (h * w)

    for kstar in (-9, -2, 3):
        for targets in (between(0, kstar), [between(0, kstar), between(1, kstar + 4)]):
            blob = model.compress(x, target_bpp=targets, step_offsets=off)
            rep = model.last_compress_report
            budgets = ec.check_budgets(targets, n) * h * w
            want = [min(k for k in ladder if at(i, k) <= budgets[i]) for i in range(n)]          # the rule, restated
            assert want[0] == kstar and (np.ndim(targets) == 0 or want[1] == kstar + 4)
            pay, hd = payload_bits(model, blob)
            for i in range(n):
                print(f"\ntarget {budgets[i] / (h * w):.4f} bpp image {i}: base {rep[i]['step_chosen']}, predicted {rep[i]['bits_predicted']:.1f}, "
                      f"payload {pay[i]:.0f} + map {rep[i]['map_bits']:.0f}, budget {budgets[i]:.1f} bits")
                assert rep[i]["step_chosen"] == want[i] and rep[i]["met"] is True and rep[i]["map_bits"] == map_bits[i]
                assert rep[i]["bits_predicted"] == at(i, want[i]) and rep[i]["budget_bits"] == budgets[i]
                assert pay[i] + map_bits[i] <= budgets[i] + slack_bar(model, hd)
            assert blob[4] == 7 and (hd["kmap"] == ec.index_map(want, off)).all()
            assert 8 * len(ec.pack_runs(hd["kmap"].reshape(n, -1))) <= map_bits.sum()               # the bound on the records
            assert blob == model.compress(x, step=want, step_offsets=off)
    # a budget nothing meets: the coarsest base, reported as not met, and the file still decodes
    blob = model.compress(x, target_bpp=0.5 * float(bits[:, -1].min()) / (h * w), step_offsets=off)
    rep = model.last_compress_report
    assert [r["step_chosen"] for r in rep] == [ec.STEP_MAX] * n and not any(r["met"] for r in rep)
    assert [r["bits_predicted"] for r in rep] == bits[:, -1].tolist()
    px = model.decompress(blob)
    assert tuple(px.shape) == (n, h, w, 3) and torch.equal(px, model.decompress(model.compress(x, step=ec.STEP_MAX, step_offsets=off)))
    # all-zero offsets: today's rate control and report
    t = between(0, 3)
    assert model.compress(x, target_bpp=t, step_offsets=np.zeros_like(off)) == model.compress(x, target_bpp=t)
    assert all("map_bits" not in r for r in model.last_compress_report)


def test_refusals(dev, hyper_model, fact_model, monkeypatch):
    from shallow_ntc_amd import _capi as capi
    from shallow_ntc_amd.mshyper.models import Model
    from test_hip_sga import TC
    model = hyper_model
    x = images(2, 64, 64, dev)
    hh, ww = model.step_offsets_shape(64, 64)
    off = np.zeros((2, hh, ww), np.int8)
    off[:, 0, 0] = 9
    blob = model.compress(x, step_offsets=off)
    assert blob[4] == 7
    with pytest.raises(capi.SntcError) as e:                    # a factorized model reads v4 only
        fact_model.decompress(blob)
    assert e.value.code == capi.ERR_UNSUPPORTED
    forged = bytearray(blob)
    forged[4] = 6                                               # version 6 stays refused
    with pytest.raises(capi.SntcError) as e:
        model.decompress(bytes(forged))
    assert e.value.code == capi.ERR_UNSUPPORTED
    launches = []
    for m in (model, fact_model):
        analysis = m.infer_latent_rvs
        monkeypatch.setattr(m, "infer_latent_rvs", lambda *a, _f=analysis, **k: launches.append(1) or _f(*a, **k))
    with pytest.raises(ValueError, match="itinf"):
        model.compress(x, itinf=dict(steps=2), step_offsets=off)
    with pytest.raises(ValueError, match="exclude"):
        model.compress(x, step=1, target_bpp=0.3, step_offsets=off)
    z_hat, sym = torch.zeros((2, 1, 1, 192), device=dev), torch.zeros((2, hh, ww, 320), dtype=torch.int32, device=dev)
    for bad in (off[:1], off[:, :-1], off[0], off.astype(np.float32), off > 0, off + 65, off - 74, off.astype(np.float64).tolist(), "map"):
        with pytest.raises(ValueError):
            model.compress(x, step_offsets=bad)
        with pytest.raises(ValueError):
            model.compress(x, target_bpp=0.3, step_offsets=bad)
        with pytest.raises(ValueError):
            model.coded_cost(x, step_offsets=bad)
        with pytest.raises(ValueError):
            model.decode(z_hat, sym, (64, 64), step_offsets=bad)
    with pytest.raises(ValueError):
        model.compress(x, step=33, step_offsets=off)
    for kw in (dict(step_offsets=off), dict(step=1, step_offsets=off), dict(target_bpp=0.3, step_offsets=off)):
        with pytest.raises(NotImplementedError, match="factorized"):
            fact_model.compress(x, **kw)
    with pytest.raises(NotImplementedError, match="factorized"):
        fact_model.coded_cost(x, step_offsets=off)
    with pytest.raises(NotImplementedError, match="factorized"):
        fact_model.step_offsets_shape(64, 64)
    with pytest.raises(NotImplementedError, match="factorized"):
        fact_model.decode(torch.zeros((1, 4, 4, 8), device=dev), None, (64, 64), step_offsets=off)
    split = Model(device=dev, rd_lambda=0.02, transform_config=TC, precision="bf16x3")
    monkeypatch.setattr(split, "infer_latent_rvs", lambda *a, **k: launches.append(1))
    for kw in (dict(step_offsets=off), dict(target_bpp=0.3, step_offsets=off)):
        with pytest.raises(NotImplementedError, match="bf16x3"):
            split.compress(x, **kw)
    with pytest.raises(NotImplementedError, match="bf16x3"):
        split.coded_cost(x, step_offsets=off)
    with pytest.raises(NotImplementedError, match="bf16x3"):
        split.decode(z_hat, sym, (64, 64), step_offsets=off)
    assert not launches                                         # every refusal came before the analysis ran
