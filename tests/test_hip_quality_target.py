"""Quality-targeted compress (-m gpu; DESIGN.md 4.7, "quality target"): the ladder-dequantisation kernels of
csrc/quant_step.hip against the float32 rule in NumPy (bit equality) and against the per-step kernels, ``ladder_distortion``
against ``coded_cost`` (integer equality), ``rd_curve``, and ``compress(x, target_psnr=...)`` against ``compress(x, step=...)``
(byte equality) and a brute-force restatement of the rule."""
from fractions import Fraction

import ctypes as C
import numpy as np
import pytest
import torch

from test_hip_itinf_bitstream import fact_model, hyper_model, images  # noqa: F401
from test_hip_quant_step import LADDERS, N, case_of, dev_case, dv, latents, np_step_symbols, round_f32, sse_of
from test_hip_step_map import np_map_symbols, offsets_for

pytestmark = pytest.mark.gpu

# (E, c, stride) of test_hip_quant_step.make_case (3 images): the vector path over two workgroup passes' worth of units; mu rows
# of 2 c floats; c % 4 != 0 (the element-wise path); the model's width
CASES = [(1028, 4, 4), (4100, 4, 8), (963, 3, 3), (960, 320, 640)]
KERNEL_LADDERS = [[-32], [32], LADDERS[4]]                  # 1 and 16 candidates, indexes spanning -32 .. 32
assert len(LADDERS[4]) == 16 and LADDERS[4][0] == -32 and LADDERS[4][-1] == 32


def np_fma_f32(step, s, mu):
    """fmaf(step, (float)s, mu): float32(mu + step * float32(s)), rounded ONCE.  The product of two float32 is exact in float64;
    the float64 sum is brought to round-to-odd with the error term of TwoSum (the inexact even result moves to its odd
    neighbour on the error's side), after which rounding 53 bits to 24 is the correct rounding of the exact value."""
    prod = np.float64(step) * s.astype(np.float32).astype(np.float64)
    m = mu.astype(np.float64)
    t = m + prod
    bb = t - m
    err = (m - (t - bb)) + (prod - bb)
    even = (t.view(np.int64) & 1) == 0
    t = np.where((err != 0) & even, np.nextafter(t, np.where(err > 0, np.inf, -np.inf)), t)
    return t.astype(np.float32)


def np_ladder_values(cs, ks):
    """[len(ks), N, hw, c] float32: the three lines of np_step_symbols and one fma per candidate."""
    from shallow_ntc_amd import entropy_coding as ec
    out = []
    for k in ks:
        sym, _, _ = np_step_symbols(cs["y"], cs["mu"], cs["ids"], [k] * N)
        out.append(np_fma_f32(np.float32(ec.step_size(k)), sym, cs["mu"]))
    return np.stack(out)


def offset_view(t, dev):
    """The same values one float into an allocation of their own: 4-byte aligned, not 16."""
    v = torch.cat([torch.zeros(1, dtype=t.dtype, device=dev), t.flatten()])[1:].view(t.shape)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


_want = {}


def want_of(key, ks):
    """The NumPy reference of a case and ladder, computed once and shared."""
    k = (key, tuple(ks))
    if k not in _want:
        _want[k] = np_ladder_values(case_of(*key), ks)
    return _want[k]


def test_the_float64_emulation_is_one_rounding():
    """np_fma_f32 against exact rational arithmetic on elements chosen to include ties of the float64 sum's low bits."""
    from shallow_ntc_amd import entropy_coding as ec
    cs = case_of(4100, 4, 8)
    for k in (-32, 5, 32):
        sym, _, _ = np_step_symbols(cs["y"], cs["mu"], cs["ids"], [k] * N)
        got = np_fma_f32(np.float32(ec.step_size(k)), sym, cs["mu"]).reshape(-1)
        s, m = sym.reshape(-1), np.ascontiguousarray(cs["mu"]).reshape(-1)
        for j in list(range(300)) + list(range(len(s) - 60, len(s))):
            want = round_f32(Fraction(float(m[j])) + Fraction(ec.step_size(k)) * Fraction(float(np.float32(s[j]))))
            assert got[j].view(np.uint32) == want.view(np.uint32), (k, j)


# ------------------------------------------------------------------ kernels ------------------------------------------------
@pytest.mark.parametrize("E,c,stride", CASES, ids=[f"E{E}-c{c}-stride{s}" for E, c, s in CASES])
def test_ladder_dequant_is_the_float32_rule(E, c, stride, dev):
    from shallow_ntc_amd import entropy_coding as ec
    from shallow_ntc_amd import ops
    cs = case_of(E, c, stride)
    y, hyper, ids = dev_case(cs, dev)
    for ks in KERNEL_LADDERS:
        st, inv, sh = ec.step_tensors(ks, dev)
        got = ops.step_ladder_dequant(y, hyper, inv, st)
        assert got.dtype == torch.float32 and tuple(got.shape) == (len(ks),) + tuple(y.shape) and got.is_contiguous()
        want = want_of((E, c, stride), ks)
        np.testing.assert_array_equal(got.cpu().numpy().reshape(want.shape).view(np.uint32), want.view(np.uint32))
        if c % 4 == 0:                                       # each plane: the per-step kernels at that step, bit for bit
            for j, k in enumerate(ks):
                s1, i1, h1 = ec.step_tensors([k] * N, dev)
                sym, _ = ops.step_symbols(y, hyper, ids, i1, h1)
                assert torch.equal(got[j].view(torch.int32), ops.dequant_step(sym, hyper, s1).view(torch.int32)), k
    # the inputs exercise what they claim: at the finest step symbols pass the file's 16-bit escape on both sides, unclamped
    sym = np_step_symbols(cs["y"], cs["mu"], cs["ids"], [-32] * N)[0]
    assert (sym > 32767).any() and (sym < -32768).any()


@pytest.mark.parametrize("E,c,stride", [(1028, 4, 4), (960, 320, 640)])
def test_ladder_dequant_from_offset_views(E, c, stride, dev):
    """y, mu and the output each one float into their allocation: the element-wise path on sizes that would take 16-byte
    accesses, the same bits."""
    from shallow_ntc_amd import entropy_coding as ec
    from shallow_ntc_amd import ops
    cs = case_of(E, c, stride)
    y, hyper, _ = dev_case(cs, dev)
    ks = KERNEL_LADDERS[2]
    st, inv, _ = ec.step_tensors(ks, dev)
    want = want_of((E, c, stride), ks)
    y2, h2 = offset_view(y, dev), offset_view(hyper, dev)
    for a, b, own in ((y2, hyper, False), (y, h2, False), (y, hyper, True), (y2, h2, True)):
        out = offset_view(torch.full((len(ks),) + tuple(y.shape), -7.0, device=dev), dev) if own else None
        got = ops.step_ladder_dequant(a, b, inv, st, out=out)
        assert out is None or got is out
        np.testing.assert_array_equal(got.cpu().numpy().reshape(want.shape).view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("c", [4, 320])
def test_map_ladder_dequant(c, dev):
    """Candidate j at clip(base[j] + offsets): the NumPy rule, and dequant_step_map of step_map_symbols on that map, for 1 and
    16 bases, offsets that include +-64 (the clamp at both ends of the table), mu rows of c and of 2 c floats, and the
    element-wise path."""
    from shallow_ntc_amd import entropy_coding as ec
    from shallow_ntc_amd import ops
    n, hw = 2, 35
    rng = np.random.default_rng(c)
    lut = ec.step_lut(dev)
    off = rng.integers(-40, 41, size=(n, hw)).astype(np.int8)
    off[:, 0], off[:, 1], off[:, -1], off[:, 2] = 64, -64, 64, 0
    rows = (rng.standard_normal((n, hw, 2 * c)) * 2.0).astype(np.float32)
    mu = rows[..., :c]
    y = (mu + rng.standard_normal((n, hw, c)) * np.exp(rng.uniform(-2.0, 4.0, (n, hw, c)))).astype(np.float32)
    y[:, 1, -2:] += np.array([30000.0, -30000.0], np.float32)                     # far outside every table, at the finest step
    ids = rng.integers(0, 64, size=(n, hw, c)).astype(np.int16)
    yd, idd, offd = dv(y, dev).unsqueeze(2), dv(ids, dev).unsqueeze(2), dv(off, dev).unsqueeze(2)
    for hyper in (dv(rows, dev).unsqueeze(2), dv(mu, dev).unsqueeze(2)):
        for bases in ([-32], [0], LADDERS[4]):
            bd = torch.tensor(bases, dtype=torch.int32).to(dev)
            got = ops.step_map_ladder_dequant(yd, hyper, offd, lut, bd)
            assert tuple(got.shape) == (len(bases), n, hw, 1, c)
            for j, b in enumerate(bases):
                K = np.clip(b + off.astype(np.int64), -32, 32)
                sym, _, _ = np_map_symbols(y, mu, ids, K)
                step = np.array([ec.step_size(int(k)) for k in range(-32, 33)], np.float32)[K + 32][..., None]
                want = np_fma_f32(np.broadcast_to(step, sym.shape), sym, mu)
                np.testing.assert_array_equal(got[j].cpu().numpy().reshape(want.shape).view(np.uint32), want.view(np.uint32))
                kd = dv(K.astype(np.int8), dev).unsqueeze(2)
                dsym, _ = ops.step_map_symbols(yd, hyper, idd, kd, lut)
                assert torch.equal(got[j].view(torch.int32), ops.dequant_step_map(dsym, hyper, kd, lut).view(torch.int32)), b
            assert torch.equal(ops.step_map_ladder_dequant(offset_view(yd, dev), offset_view(hyper, dev), offd, lut, bd), got)
    assert (np.clip(-32 + off.astype(int), -32, 32) != -32 + off.astype(int)).any() and (np.clip(32 + off.astype(int), -32, 32) != 32 + off.astype(int)).any()
    # zero offsets: the per-image ladder kernel at those steps
    st, inv, _ = ec.step_tensors(LADDERS[4], dev)
    assert torch.equal(ops.step_map_ladder_dequant(yd, hyper, torch.zeros_like(offd), lut, bd), ops.step_ladder_dequant(yd, hyper, inv, st))


def test_kernel_refusals(dev):
    """Every refusal is SNTC_ERR_BAD_SHAPE before any launch: nothing is written to a sentinel-filled output."""
    from shallow_ntc_amd import _capi as capi
    from shallow_ntc_amd import entropy_coding as ec
    from shallow_ntc_amd import ops
    n, hw, c = 2, 5, 8
    y = torch.zeros((n, hw, 1, c), dtype=torch.float32, device=dev)
    mu2 = torch.zeros((n, hw, 1, 2 * c), dtype=torch.float32, device=dev)
    st, inv, sh = ec.step_tensors(list(range(-8, 9)), dev)                  # 17 entries
    lut = ec.step_lut(dev)
    off = torch.zeros((n, hw, 1), dtype=torch.int8, device=dev)
    out = torch.full((17, n, hw, 1, c), -7.0, dtype=torch.float32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    null = C.c_void_p(0)
    stream = ops._stream()

    def plain(yp=p(y), mp=p(y), vp=p(inv), sp=p(st), k=5, nn=n, cc=c, stride=c, op=p(out)):
        capi.call("sntc_step_ladder_dequant", yp, mp, nn, hw, cc, stride, vp, sp, k, op, stream)

    def mapped(yp=p(y), mp=p(y), fp=p(off), lp=p(lut), bp=p(sh), k=5, nn=n, cc=c, stride=c, op=p(out)):
        capi.call("sntc_step_map_ladder_dequant", yp, mp, nn, hw, cc, stride, fp, lp, bp, k, op, stream)

    bad = []
    for fn, pointers in ((plain, ("yp", "mp", "vp", "sp", "op")), (mapped, ("yp", "mp", "fp", "lp", "bp", "op"))):
        bad += [(fn, dict(k=0)), (fn, dict(k=17)), (fn, dict(k=-1)), (fn, dict(nn=0)), (fn, dict(nn=65536)), (fn, dict(cc=0, stride=0)),
                (fn, dict(stride=c + 4)), (fn, dict(stride=3 * c)), (fn, dict(stride=c // 2))]
        bad += [(fn, {name: null}) for name in pointers]
    for fn, kw in bad:
        with pytest.raises(capi.SntcError) as e:
            fn(**kw)
        assert e.value.code == capi.ERR_BAD_SHAPE and "ladder_dequant" in str(e.value), kw
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())                                        # no refused call launched anything
    # the same calls with good arguments run: 16 candidates, one candidate, mu rows of 2 c floats
    plain(k=16), plain(k=1), plain(mp=p(mu2), stride=2 * c), mapped(k=16), mapped(mp=p(mu2), stride=2 * c)
    torch.cuda.synchronize()
    assert bool((out[:16] == 0.0).all()) and bool((out[16] == -7.0).all())
    with pytest.raises(capi.SntcError):                                     # through the wrapper: 17 candidates
        ops.step_ladder_dequant(y, mu2, inv, st)
    with pytest.raises(capi.SntcError):
        ops.step_ladder_dequant(y, mu2, inv[:0], st[:0])


# ------------------------------------------------------------------ codec --------------------------------------------------
STEPS = [-6, -1, 0, 3, 9]
SHAPES = [(2, 128, 128), (1, 200, 120)]


@pytest.mark.parametrize("n,h,w", SHAPES)
def test_ladder_distortion_is_coded_cost(n, h, w, dev, hyper_model):
    """Integer equality with one coded_cost per step, whatever the chunking and the batching."""
    model = hyper_model
    codec = model._get_codec()
    x = images(n, h, w, dev)
    z, y = latents(model, x)
    sse = codec.ladder_distortion(z, y, x, STEPS)
    assert sse.dtype == torch.int64 and tuple(sse.shape) == (n, len(STEPS)) and sse.is_cuda
    sse = sse.cpu().numpy()
    for j, k in enumerate(STEPS):
        want = model.coded_cost(x, step=k)["sse"]
        print(f"\n{n}x{h}x{w} step {k}: sse {sse[:, j].tolist()}")
        assert sse[:, j].tolist() == want.astype(np.int64).tolist(), k
    assert len({tuple(col) for col in sse.T[:3]}) == 3                               # the steps really decode to different pixels
    # one candidate per decoder batch; two; a pre-computed hyper-synthesis
    assert codec.ladder_distortion(z, y, x, STEPS, chunk_bytes=1).cpu().numpy().tolist() == sse.tolist()
    assert codec.ladder_distortion(z, y, x, STEPS, chunk_bytes=2 * 4 * y.numel()).cpu().numpy().tolist() == sse.tolist()
    assert codec.ladder_distortion(z, y, x, STEPS, pre=codec._hyper_of(z)).cpu().numpy().tolist() == sse.tolist()
    # the images one at a time
    for i in range(n):
        assert codec.ladder_distortion(z[i:i + 1], y[i:i + 1], x[i:i + 1], STEPS).cpu().numpy().tolist() == sse[i:i + 1].tolist()
    # more candidates than one launch takes
    whole = list(range(-32, 33, 4)) + STEPS
    got = codec.ladder_distortion(z, y, x, whole).cpu().numpy()
    assert got[:, -len(STEPS):].tolist() == sse.tolist()
    # offsets that vary inside an image
    off = offsets_for(model, n, h, w)
    got = codec.ladder_distortion(z, y, x, STEPS, step_offsets=off).cpu().numpy()
    for j, k in enumerate(STEPS):
        assert got[:, j].tolist() == model.coded_cost(x, step=k, step_offsets=off)["sse"].astype(np.int64).tolist(), k
    assert got.tolist() != sse.tolist()
    assert codec.ladder_distortion(z, y, x, STEPS, step_offsets=off, chunk_bytes=1).cpu().numpy().tolist() == got.tolist()


@pytest.mark.parametrize("n,h,w", SHAPES)
def test_rd_curve(n, h, w, dev, hyper_model):
    model = hyper_model
    codec = model._get_codec()
    x = images(n, h, w, dev)
    rd = model.rd_curve(x, steps=STEPS)
    assert rd["steps"] == STEPS and rd["bits"].shape == (n, len(STEPS)) and rd["bits"].dtype == np.float64
    assert rd["sse"].dtype == np.int64 and rd["flushed_bits"] == float(codec.flushed_bits(h, w))
    for j, k in enumerate(STEPS):
        cost = model.coded_cost(x, step=k)
        assert rd["bits"][:, j].tolist() == (cost["bits"] + codec.flushed_bits(h, w)).tolist(), k
        assert rd["sse"][:, j].tolist() == cost["sse"].astype(np.int64).tolist() and rd["bits_z"].tolist() == cost["bits_z"].tolist()
    assert rd["bpp"].tolist() == (rd["bits"] / (h * w)).tolist()
    assert rd["psnr"].tolist() == (10.0 * np.log10(255.0 ** 2 * 3 * h * w / rd["sse"].astype(np.float64))).tolist()
    off = offsets_for(model, n, h, w)
    rd = model.rd_curve(x, steps=STEPS, step_offsets=off)
    for j, k in enumerate(STEPS):
        cost = model.coded_cost(x, step=k, step_offsets=off)
        assert rd["bits"][:, j].tolist() == (cost["bits"] + codec.flushed_bits(h, w)).tolist(), k
        assert rd["sse"][:, j].tolist() == cost["sse"].astype(np.int64).tolist()
    from shallow_ntc_amd import entropy_coding as ec
    assert rd["map_bits"].tolist() == (24.0 * ec.count_runs(off)).tolist()


def brute_force(bits, sse, budget, ladder):
    """The rule restated: among the steps within the budget the fewest bits, the larger index on equal bits."""
    ok = [j for j in range(len(ladder)) if sse[j] <= budget]
    return max(ok, key=lambda j: (-bits[j], ladder[j])) if ok else None


def target_from_curve(rd, i, ladder, h, w):
    """A PSNR target at the midpoint between two adjacent values of image i's curve whose brute-force choice is an interior step
    of the ladder (searched from the middle of the curve outwards; the middle one where no midpoint has an interior choice):
    -> (target dB, the chosen position)."""
    from shallow_ntc_amd import entropy_coding as ec
    vals = np.unique(rd["psnr"][i][np.isfinite(rd["psnr"][i])])
    mids = 0.5 * (vals[1:] + vals[:-1])
    mids = mids[np.argsort(np.abs(mids - np.median(vals)), kind="stable")]
    choice = lambda q: brute_force(rd["bits"][i], rd["sse"][i], ec.quality_budgets([q], h, w)[0], ladder)
    for q in mids:
        j = choice(q)
        if ec.STEP_MIN < ladder[j] < ec.STEP_MAX:
            return float(q), j
    return float(mids[0]), choice(mids[0])


def test_target_psnr(dev, hyper_model):
    from shallow_ntc_amd import entropy_coding as ec
    model = hyper_model
    codec = model._get_codec()
    n, h, w = 2, 128, 128
    x = images(n, h, w, dev)
    rd = model.rd_curve(x)
    ladder = rd["steps"]
    assert ladder == list(range(ec.STEP_MIN, ec.STEP_MAX + 1))
    for i in range(n):
        print(f"\nimage {i}: psnr {np.round(rd['psnr'][i][::8], 3).tolist()} dB, bits {np.round(rd['bits'][i][::8]).tolist()} at steps {ladder[::8]}")
    picks = [target_from_curve(rd, i, ladder, h, w) for i in range(n)]
    # one target for the batch (image 0's), then per-image targets that choose independently
    for targets in (picks[0][0], [q for q, _ in picks]):
        blob = model.compress(x, target_psnr=targets)
        rep = model.last_compress_report
        budgets = ec.quality_budgets(ec.check_quality(targets, n), h, w)
        chosen = [r["step_chosen"] for r in rep]
        for i in range(n):
            j = brute_force(rd["bits"][i], rd["sse"][i], budgets[i], ladder)
            print(f"\ntarget {ec.check_quality(targets, n)[i]:.3f} dB image {i}: step {chosen[i]}, predicted {rep[i]['bits_predicted']:.1f} bits, "
                  f"{rep[i]['psnr_predicted']:.3f} dB, sse {rep[i]['sse_predicted']:.0f} <= {budgets[i]:.1f}")
            assert rep[i]["met"] is True and chosen[i] == ladder[j] and (np.ndim(targets) == 0 and i > 0 or j == picks[i][1])
            assert rep[i]["bits_predicted"] == rd["bits"][i, j] and rep[i]["sse_predicted"] == rd["sse"][i, j]
            assert rep[i]["sse_budget"] == budgets[i] and rep[i]["psnr_predicted"] == rd["psnr"][i, j] >= ec.check_quality(targets, n)[i]
            # every step of the ladder with fewer predicted bits misses the budget
            assert all(rd["sse"][i, t] > budgets[i] for t in range(len(ladder)) if rd["bits"][i, t] < rd["bits"][i, j])
        assert ec.STEP_MIN < chosen[0] < ec.STEP_MAX                                 # image 0's target was chosen for an interior step
        assert blob == model.compress(x, step=chosen)
        assert codec._parse(blob)["steps"] == (chosen if any(chosen) else None)
        got = sse_of(model.decompress(blob), x)
        assert got.tolist() == [int(r["sse_predicted"]) for r in rep] and (got <= budgets).all()
    # a target nothing reaches: the finest step, reported as not met, and the file is that step's
    blob = model.compress(x, target_psnr=200.0)
    rep = model.last_compress_report
    assert [r["step_chosen"] for r in rep] == [ec.STEP_MIN] * n and not any(r["met"] for r in rep)
    assert [r["sse_predicted"] for r in rep] == rd["sse"][:, 0].tolist() and [r["bits_predicted"] for r in rep] == rd["bits"][:, 0].tolist()
    assert blob == model.compress(x, step=ec.STEP_MIN)
    # a target everything reaches: the cheapest step of the ladder
    model.compress(x, target_psnr=-50.0)
    for i, r in enumerate(model.last_compress_report):
        assert r["met"] and r["bits_predicted"] == rd["bits"][i].min()


def test_target_psnr_with_offsets(dev, hyper_model):
    from shallow_ntc_amd import entropy_coding as ec
    model = hyper_model
    n, h, w = 2, 128, 128
    x = images(n, h, w, dev)
    off = offsets_for(model, n, h, w)
    rd = model.rd_curve(x, step_offsets=off)
    ladder = rd["steps"]
    picks = [target_from_curve(rd, i, ladder, h, w) for i in range(n)]
    targets = [q for q, _ in picks]
    blob = model.compress(x, target_psnr=targets, step_offsets=off)
    rep = model.last_compress_report
    budgets = ec.quality_budgets(ec.check_quality(targets, n), h, w)
    chosen = [r["step_chosen"] for r in rep]
    for i in range(n):
        j = brute_force(rd["bits"][i], rd["sse"][i], budgets[i], ladder)
        assert rep[i]["met"] is True and chosen[i] == ladder[j] == ladder[picks[i][1]]
        assert rep[i]["map_bits"] == rd["map_bits"][i] and rep[i]["bits_predicted"] == rd["bits"][i, j] + rd["map_bits"][i]
        assert rep[i]["sse_predicted"] == rd["sse"][i, j]
        assert all(rd["sse"][i, t] > budgets[i] for t in range(len(ladder)) if rd["bits"][i, t] < rd["bits"][i, j])
    assert blob[4] == 7 and blob == model.compress(x, step=chosen, step_offsets=off)
    got = sse_of(model.decompress(blob), x)
    assert got.tolist() == [int(r["sse_predicted"]) for r in rep] and (got <= budgets).all()


def test_refusals(dev, hyper_model, fact_model, monkeypatch):
    from shallow_ntc_amd.mshyper.models import Model
    from test_hip_sga import TC
    model = hyper_model
    x = images(2, 64, 64, dev)
    launches = []
    for m in (model, fact_model):
        analysis = m.infer_latent_rvs
        monkeypatch.setattr(m, "infer_latent_rvs", lambda *a, _f=analysis, **k: launches.append(1) or _f(*a, **k))
    for kw in (dict(step=1), dict(target_bpp=0.3)):
        with pytest.raises(ValueError, match="exclude"):
            model.compress(x, target_psnr=30.0, **kw)
    with pytest.raises(ValueError, match="itinf"):
        model.compress(x, target_psnr=30.0, itinf=dict(steps=2))
    with pytest.raises(ValueError, match="not implemented inside itinf"):
        model.compress(x, itinf=dict(steps=2, target_psnr=30.0))
    for bad in (float("nan"), [30.0], [30.0, 31.0, 32.0], "high"):
        with pytest.raises(ValueError, match="target_psnr"):
            model.compress(x, target_psnr=bad)
    with pytest.raises(NotImplementedError, match="factorized"):
        fact_model.compress(x, target_psnr=30.0)
    with pytest.raises(NotImplementedError, match="factorized"):
        fact_model.rd_curve(x)
    split = Model(device=dev, rd_lambda=0.02, transform_config=TC, precision="bf16x3")
    monkeypatch.setattr(split, "infer_latent_rvs", lambda *a, **k: launches.append(1))
    with pytest.raises(NotImplementedError, match="bf16x3"):
        split.compress(x, target_psnr=30.0)
    with pytest.raises(NotImplementedError, match="bf16x3"):
        split.rd_curve(x)
    assert not launches                                         # every refusal came before the analysis ran
