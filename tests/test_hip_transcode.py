"""Transcoding a bitstream to a coarser quantisation step without pixels (-m gpu; DESIGN.md 4.7, "transcode").  The requantisation
kernels of csrc/quant_step.hip against the composition of the entry points they fuse (sntc_dequant_step_map, then
sntc_step_map_symbols / sntc_step_map_table_ids / sntc_step_map_ladder_cost on the stored values), bit for bit; ``transcode``
against ``compress_latents`` of the source file's decoded latents, byte for byte; rate control over shifts; the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_hip_itinf_bitstream import big_table_set, hyper_model, image_words, images  # noqa: F401
from test_hip_quant_step import N, case_of, dev_case, dv, latents, normal, offset_view  # noqa: F401
from test_hip_step_map import CASES as MAP_CASES
from test_hip_step_map import MAPS, dmap, lut, make_map, np_map_symbols, offsets_for  # noqa: F401

pytestmark = pytest.mark.gpu

CASES = [k for k in MAP_CASES if k[1] == 4]              # c = 4, hw in 1, 15, 16, 17, 255, 256, 257, 1025, mu rows of 4 and 8 floats
IDS = [f"hw{E // c}-c{c}-stride{s}" for E, c, s in CASES]
SHIFTS = [[0], [64], [0, 1, 5, 33], [0, 1, 2, 3, 4, 5, 6, 8, 11, 16, 24, 32, 33, 47, 63, 64]]


def source(cs, kind, dev):
    """A file's side of a case: the source map K0 (both ends of the ladder present where hw allows) and the symbols the file
    would hold at it -- the float32 rule on the case's y, escapes beyond every table's half-width included -- on the device."""
    K0 = make_map(kind, cs)
    s0, _, _ = np_map_symbols(cs["y"], cs["mu"], cs["ids"], K0)
    return K0, s0, dv(s0, dev).unsqueeze(2), dmap(K0, dev)


def reference_cost(y_hat, hyper, ids, K0, shifts, tables, lut, dev):
    """``step_map_ladder_cost`` on the decoded values with offsets = the source map and the shifts as its bases.  A base stops at
    32: a shift beyond it is priced with the excess moved into the offsets, clip((d - e) + (K0 + e)) = clip(K0 + d)."""
    from shallow_ntc_amd import entropy_coding as ec
    if max(shifts) <= 32:
        return ec.step_map_ladder_cost(y_hat, hyper, ids, dmap(K0, dev), shifts, tables, lut)
    cols = [ec.step_map_ladder_cost(y_hat, hyper, ids, dmap(K0.astype(np.int64) + max(d - 32, 0), dev), [min(d, 32)], tables, lut) for d in shifts]
    return torch.cat(cols, dim=1)


def check_against_the_composition(s0d, hyper, ids, K0, k0d, tables, lut, dev, shift_sets=SHIFTS):
    from shallow_ntc_amd import entropy_coding as ec
    from shallow_ntc_amd import ops
    y_hat = ops.dequant_step_map(s0d, hyper, k0d, lut)               # what decompress would feed the synthesis, stored as float32
    for d in sorted({d for s in shift_sets for d in s}):
        dst = dmap(np.clip(K0.astype(np.int64) + d, -32, 32), dev)
        want_sym, want_tid = ops.step_map_symbols(y_hat, hyper, ids, dst, lut)
        sym, tid = ops.step_requant_symbols(s0d, hyper, ids, k0d, dst, lut)
        assert sym.dtype == torch.int32 and tid.dtype == torch.int16
        assert torch.equal(sym, want_sym) and torch.equal(tid, want_tid), d
        assert torch.equal(tid, ec.step_map_table_ids(ids, dst)), d
    for shifts in shift_sets:
        got = ec.step_requant_ladder_cost(s0d, hyper, ids, k0d, shifts, tables, lut)
        assert got.dtype == torch.int64 and tuple(got.shape) == (s0d.shape[0], len(shifts))
        want = reference_cost(y_hat, hyper, ids, K0, shifts, tables, lut, dev)
        assert got.cpu().numpy().tolist() == want.cpu().numpy().tolist(), shifts
    return y_hat


# ------------------------------------------------------------------ kernels ------------------------------------------------
@pytest.mark.parametrize("E,c,stride", CASES, ids=IDS)
def test_requant_kernels_are_the_composition(E, c, stride, dev, lut, normal):
    from shallow_ntc_amd import ops
    _, dt, _ = normal
    cs = case_of(E, c, stride)
    _, hyper, ids = dev_case(cs, dev)
    for kind in MAPS:
        K0, s0, s0d, k0d = source(cs, kind, dev)
        assert (np.abs(s0) > 4096).any()                             # beyond the widest table's half-width: the escape rule prices them
        assert (K0 == -32).any() and (K0 == 32).any()                # the pinned positions, if nothing else: both ends of the ladder
        y_hat = check_against_the_composition(s0d, hyper, ids, K0, k0d, dt, lut, dev)
    # a destination that is not source + shift: any map is one (the kernel takes the two maps as they are)
    K1 = make_map("random", cs, pin=False)
    want = ops.step_map_symbols(y_hat, hyper, ids, dmap(K1, dev), lut)
    got = ops.step_requant_symbols(s0d, hyper, ids, k0d, dmap(K1, dev), lut)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_constant_maps_are_the_per_image_kernels(dev, lut, normal):
    """A unit or per-image source is a constant map: the requantised symbols are ``step_symbols`` of ``dequant_step``'s values."""
    from shallow_ntc_amd import entropy_coding as ec
    from shallow_ntc_amd import ops
    cs = case_of(1028, 4, 8)
    _, hyper, ids = dev_case(cs, dev)
    k0, k1 = [-3, 0, 4], [2, 0, 32]
    K0 = np.broadcast_to(np.array(k0)[:, None], (N, cs["hw"]))
    s0, _, _ = np_map_symbols(cs["y"], cs["mu"], cs["ids"], K0)
    s0d = dv(s0, dev).unsqueeze(2)
    st0, _, _ = ec.step_tensors(k0, dev)
    _, inv1, sh1 = ec.step_tensors(k1, dev)
    want = ops.step_symbols(ops.dequant_step(s0d, hyper, st0), hyper, ids, inv1, sh1)
    got = ops.step_requant_symbols(s0d, hyper, ids, dmap(K0, dev), dmap(np.broadcast_to(np.array(k1)[:, None], K0.shape), dev), lut)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_requant_over_several_passes(dev, lut, normal):
    """n = 3 images whose units exceed what the launch's workgroups take in one pass, by a non-multiple, on both load paths."""
    from shallow_ntc_amd import entropy_coding as ec
    _, dt, _ = normal
    n, hw, c, stride = 3, 300011, 4, 8
    for per_unit in (4, 1):
        units = hw * c // per_unit
        grid = min(-(-units // 1024), max(1, 512 // n))
        assert units > grid * 1024 and units % (grid * 1024) != 0
    rng = np.random.default_rng(n + hw + c + stride)
    ids = rng.integers(0, 64, size=(n, hw, c)).astype(np.int16)
    rows = (rng.standard_normal((n, hw, stride)) * 2.0).astype(np.float32)
    sig = 0.11 * np.exp(ec.SCALE_FACTOR * ids.astype(np.float64))
    K0 = rng.integers(-32, 33, size=(n, hw)).astype(np.int8)
    step0 = np.array([ec.step_size(k) for k in range(-32, 33)])[K0.astype(np.int64) + 32][..., None]
    s0 = np.rint(rng.standard_normal((n, hw, c)) * sig / step0 * np.where(rng.random((n, hw, c)) < 0.2, 3.5, 1.0)).astype(np.int32)
    s0.reshape(n, -1)[:, -4:] = [20000, -20000, 300, -300]                                       # escapes in the last pass
    s0d, hd, idd, k0d = dv(s0, dev).unsqueeze(2), dv(rows, dev).unsqueeze(2), dv(ids, dev).unsqueeze(2), dmap(K0, dev)
    sets = [[0, 3, 33]]
    check_against_the_composition(s0d, hd, idd, K0, k0d, dt, lut, dev, sets)
    s2, h2, i2 = offset_view(s0d, 1, dev), offset_view(hd, 1, dev), offset_view(idd, 2, dev)
    want = ec.step_requant_ladder_cost(s0d, hd, idd, k0d, sets[0], dt, lut)
    assert torch.equal(ec.step_requant_ladder_cost(s2, h2, i2, k0d, sets[0], dt, lut), want)


def test_requant_cost_with_tables_beyond_the_lds_limit(dev, lut):
    """Descriptors and costs read from global memory (84 tables; the ladder is their first 64): the same exact sums."""
    from shallow_ntc_amd import entropy_coding as ec
    db = ec.DeviceTables(big_table_set(), dev)
    cs = case_of(4100, 4, 8)
    _, hyper, ids = dev_case(cs, dev)
    K0, _, s0d, k0d = source(cs, "random", dev)
    check_against_the_composition(s0d, hyper, ids, K0, k0d, db, lut, dev, [SHIFTS[2]])


def test_requant_cost_from_an_offset_view(dev, lut, normal):
    """The symbols, mu and the ids each start 4 bytes into their allocation (the map 1 byte into its own): the element-wise load
    path (V = 1) on a size that would take the vector path, the same sums."""
    from shallow_ntc_amd import entropy_coding as ec
    _, dt, _ = normal
    cs = case_of(4100, 4, 4)
    _, hyper, ids = dev_case(cs, dev)
    K0, _, s0d, k0d = source(cs, "random", dev)
    want = ec.step_requant_ladder_cost(s0d, hyper, ids, k0d, SHIFTS[3], dt, lut)
    s2, h2, i2, k2 = offset_view(s0d, 1, dev), offset_view(hyper, 1, dev), offset_view(ids, 2, dev), offset_view(k0d, 1, dev)
    assert s2.data_ptr() % 16 == 4 and h2.data_ptr() % 16 == 4 and i2.data_ptr() % 8 == 4 and k2.data_ptr() % 2 == 1
    for a, b, cc, kk in ((s2, h2, i2, k2), (s2, hyper, ids, k0d), (s0d, h2, ids, k0d), (s0d, hyper, i2, k0d), (s0d, hyper, ids, k2)):
        assert torch.equal(ec.step_requant_ladder_cost(a, b, cc, kk, SHIFTS[3], dt, lut), want)
    check_against_the_composition(s0d, hyper, ids, K0, k0d, dt, lut, dev, [SHIFTS[3]])           # ... which are the composition's
    from shallow_ntc_amd import _capi as capi
    from shallow_ntc_amd import ops
    with pytest.raises(capi.SntcError):                              # the symbol kernel is 16-byte accesses only, like the one it mirrors
        ops.step_requant_symbols(s2, hyper, ids, k0d, k0d, lut)


def test_kernel_refusals(dev, lut, normal):
    from shallow_ntc_amd import _capi as capi
    from shallow_ntc_amd import ops
    _, dt, _ = normal
    lib = capi.load()
    n, hw, c = 2, 5, 8
    mu = torch.zeros((n, hw, 1, c), dtype=torch.float32, device=dev)
    ids = torch.zeros((n, hw, 1, c), dtype=torch.int16, device=dev)
    tid = torch.zeros_like(ids)
    kmap = torch.zeros((n, hw, 1), dtype=torch.int8, device=dev)
    shift = torch.arange(0, 17, dtype=torch.int32, device=dev)             # 17 entries
    cost = torch.zeros((n, 17), dtype=torch.int64, device=dev)
    sym = torch.zeros((n, hw, 1, c), dtype=torch.int32, device=dev)
    out = torch.zeros_like(sym)
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = ops._stream()

    def ladder(sp=p(sym), mp=p(mu), ip=p(ids), kp=p(kmap), lp=p(lut), hp=p(shift), k=5, cc=c, stride=c, mt=p(dt.meta), cq=p(dt.cost_q), cp=p(cost),
               nt=dt.ntables, nn=n):
        return lib.sntc_step_requant_ladder_cost(sp, mp, nn, hw, cc, stride, ip, kp, lp, hp, k, mt, nt, dt.total, cq, cp, stream)

    def symbols(sp=p(sym), mp=p(mu), ip=p(ids), kp=p(kmap), dp=p(kmap), lp=p(lut), op=p(out), tp=p(tid), cc=c, stride=c, nn=n):
        return lib.sntc_step_requant_symbols(sp, mp, nn, hw, cc, stride, ip, kp, dp, lp, op, tp, stream)

    assert ladder() == capi.OK and symbols() == capi.OK
    null = C.c_void_p(0)
    bad = capi.ERR_BAD_SHAPE
    assert ladder(k=0) == bad and ladder(k=17) == bad and ladder(k=16) == capi.OK and ladder(k=1) == capi.OK
    assert ladder(cc=6, stride=6) == bad and symbols(cc=6, stride=6) == bad
    assert ladder(cc=2, stride=4) == bad and ladder(stride=4) == bad and ladder(stride=10) == bad and ladder(nt=63) == bad
    assert ladder(nn=0) == bad and ladder(nn=65536) == bad and symbols(nn=0) == bad and symbols(nn=65536) == bad
    for name in ("sp", "mp", "ip", "kp", "lp", "hp", "mt", "cq", "cp"):
        assert ladder(**{name: null}) == bad, name
    for name in ("sp", "mp", "ip", "kp", "dp", "lp", "op", "tp"):
        assert symbols(**{name: null}) == bad, name
    room = torch.zeros((n * hw * c + 4,), dtype=torch.int32, device=dev)
    odd = C.c_void_p(room.data_ptr() + 4)                               # 4 bytes in: fine for the ladder, refused by the vector kernel
    assert ladder(sp=odd) == capi.OK and symbols(sp=odd) == bad and symbols(tp=C.c_void_p(tid.data_ptr() + 4)) == bad
    torch.cuda.synchronize()
    assert "sntc_step_requant" in capi.last_error()
    # the wrappers refuse a map, a table or a shift list of the wrong shape / dtype before the call
    for km, lt in ((kmap[:, :4], lut), (kmap.to(torch.int32), lut), (kmap.cpu(), lut), (kmap, lut[:, :64]), (kmap, lut.double())):
        with pytest.raises(ValueError):
            ops.step_requant_symbols(sym, mu, ids, km, kmap, lt)
        with pytest.raises(ValueError):
            ops.step_requant_symbols(sym, mu, ids, kmap, km, lt)
        with pytest.raises(ValueError):
            ops.step_requant_ladder_cost(sym, mu, ids, km, lt, shift[:3], dt)
    for sh in (shift, shift[:0], shift[:3].to(torch.int64), shift[:3].cpu()):
        with pytest.raises(ValueError):
            ops.step_requant_ladder_cost(sym, mu, ids, kmap, lut, sh, dt)
    with pytest.raises(ValueError):
        ops.step_requant_symbols(sym.float(), mu, ids, kmap, kmap, lut)


# ------------------------------------------------------------------ files --------------------------------------------------
SIZES = [(64, 64), (96, 80)]
_files = {}


def source_file(model, kind, H, W, dev):
    """One source per (grid kind, size), shared by the tests: n = 3 images, the blob, what it holds and decodes to (the encoder's
    side of ``compress``: ``decompress`` is ``decode`` of exactly these, test_hip_quant_step / test_hip_step_map) -- z_hat, the
    file's symbols, y_hat0 = the latents the synthesis would be fed, the source indexes K0 [n, h, w]."""
    from shallow_ntc_amd import entropy_coding as ec
    key = (kind, H, W)
    if key not in _files:
        codec = model._get_codec()
        x = images(3, H, W, dev, seed=5 + H)
        h, w = model.step_offsets_shape(H, W)
        if kind == "unit":
            kw, K0 = dict(), np.zeros((3, h, w), np.int64)
        elif kind == "image":
            kw, K0 = dict(step=[-3, 0, 4]), np.broadcast_to(np.array([-3, 0, 4]).reshape(3, 1, 1), (3, h, w)).astype(np.int64)
        else:
            off = offsets_for(model, 3, H, W)
            kw, K0 = dict(step=[-3, 0, 4], step_offsets=off), np.clip(np.array([-3, 0, 4]).reshape(3, 1, 1) + off.astype(np.int64), -32, 32)
        blob = model.compress(x, **kw)
        assert blob[4] == {"unit": 3, "image": 5, "map": 7}[kind]
        z, y = latents(model, x)
        grid = ec.StepGrid.resolve(0, K0.astype(np.int8), 3, h, w)
        assert grid.kind == kind
        zi, _, sym, _, hyper = codec._symbols(z, y, grid)
        _files[key] = dict(x=x, blob=blob, z_hat=ec.int_to_float(zi), sym=sym, hyper=hyper, y_hat0=grid.dequant(sym, hyper), K0=K0, hw=(H, W))
    return _files[key]


def reference_file(model, src, K1):
    """``compress_latents(z_hat, y_hat0, (H, W))`` on the grid K1: the specification."""
    return model._get_codec().compress_latents(src["z_hat"], src["y_hat0"], src["hw"], step=0, step_offsets=K1.astype(np.int8))


def z_streams(model, blob):
    hd = model._get_codec()._parse(blob)
    return hd["zl"].tolist(), bytes(blob[hd["pos"]:hd["pos"] + 2 * hd["zw"]]), (hd["sz"], hd["lz"])


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("kind", ["unit", "image", "map"])
def test_transcode_is_compress_latents_of_the_decoded_latents(kind, H, W, dev, hyper_model):
    from shallow_ntc_amd import entropy_coding as ec
    model = hyper_model
    codec = model._get_codec()
    src = source_file(model, kind, H, W, dev)
    K0 = src["K0"]
    n, h, w = K0.shape
    assert torch.equal(model.decompress(src["blob"]), model.decode(src["z_hat"], src["sym"], (H, W), step=0, step_offsets=K0.astype(np.int8)))
    for d in (0, 1, 5, [0, 7, 2], [40, 3, 0], 64):
        ds = np.array(ec.check_shifts(d, n)).reshape(n, 1, 1)
        K1 = np.clip(K0 + ds, -32, 32)
        out = model.transcode(src["blob"], shift=d)
        want = reference_file(model, src, K1)
        assert out == want, (kind, d)
        constant = all(len(np.unique(k)) == 1 for k in K1)
        assert out[4] == (7 if not constant else 5 if K1.any() else 3)
        hd = codec._parse(out)
        assert (ec.StepGrid.from_header(hd).indexes(h, w) == K1).all()
        # the z streams, their lengths and their segment / lane fields are the source's
        assert z_streams(model, out) == z_streams(model, src["blob"])
        for i in range(n):
            assert image_words(model, out, i)[0] == image_words(model, src["blob"], i)[0]
        # what it decodes to: decode of the requantised symbols on the new grid
        s1 = codec._symbols(src["z_hat"], src["y_hat0"], ec.StepGrid.resolve(0, K1.astype(np.int8), n, h, w))[2]
        px = model.decompress(out)
        assert torch.equal(px, model.decode(src["z_hat"], s1, (H, W), step=0, step_offsets=K1.astype(np.int8))), (kind, d)
        if d == 64:                                                  # every position at the ladder's top
            assert (K1 == 32).all() and out[4] == 5 and hd["steps"] == [32] * n
            assert out == codec.compress_latents(src["z_hat"], src["y_hat0"], (H, W), step=32)
    # the symbols really moved: a coarser file is a smaller one
    assert len(model.transcode(src["blob"], shift=8)) < len(src["blob"])


def test_transcode_many_of_mixed_versions(dev, hyper_model):
    model = hyper_model
    blobs = [source_file(model, kind, H, W, dev)["blob"] for kind, (H, W) in (("unit", SIZES[0]), ("map", SIZES[1]), ("image", SIZES[0]),
                                                                             ("map", SIZES[0]))]
    assert [b[4] for b in blobs] == [3, 7, 5, 7]
    assert model.transcode_many([], shift=1) == []
    for shift in (3, [0, [1, 2, 3], 64, [0, 0, 9]]):
        many = model.transcode_many(blobs, shift=shift)
        each = [shift] * 4 if isinstance(shift, int) else shift
        assert many == [model.transcode(b, shift=s) for b, s in zip(blobs, each)]
    assert model._get_codec().transcode(blobs[1], shift=[1, 2, 3]) == model.transcode(blobs[1], shift=[1, 2, 3])
    with pytest.raises(ValueError):
        model.transcode_many(blobs, shift=[1, 2])                    # one entry per blob
    with pytest.raises(ValueError):
        model.transcode(blobs[0], shift=[1, 2])                      # one entry per image


@pytest.mark.parametrize("kind", ["image", "map"])
def test_target_bpp_picks_the_smallest_shift_that_fits(kind, dev, hyper_model):
    """The rule against the files themselves: every candidate d is written, and the chosen d is the smallest whose file fits.
    The prediction counts what ``compress(target_bpp=)`` counts: the exact cost of the symbols + the flushed lane states + M,
    M = 24 bits per run of the source map -- not the header, the length fields or the coder's word granularity.  A written
    file's payload (its streams' words) lies within ``slack`` = 16 bits per flushed lane state of cost + flushed bits (the bar
    of test_file_payload_against_the_cost), so the prediction of shift d lies in [payload(d) + M - slack, payload(d) + M + slack],
    whatever the code does.  A budget B = max(file(d*), payload(d*) + M + slack) + 1 is therefore met at d* by file and
    prediction alike, and it is used only at shifts d* where every smaller shift's file AND lower bound lie above it: there the
    smallest file that fits and the smallest prediction that fits are the same shift by arithmetic, and the test asserts the
    code found it.  The sources are fine-step files (ladder index around -24): neighbouring shifts are then further apart
    than the uncounted bits, which they are not at step 0 on images this small."""
    from shallow_ntc_amd import entropy_coding as ec
    model = hyper_model
    codec = model._get_codec()
    H, W = SIZES[1]
    x = images(3, H, W, dev, seed=5 + H)
    h, w = model.step_offsets_shape(H, W)
    off = None if kind == "image" else np.clip(offsets_for(model, 3, H, W), -6, 6).astype(np.int8)
    blob3 = model.compress(x, step=-24, step_offsets=off)
    blob = model.compress(x[1:2], step=-24, step_offsets=None if off is None else off[1:2])     # image 1 alone: a file's size is its size
    assert blob[4] == blob3[4] == (5 if kind == "image" else 7)
    assert image_words(model, blob, 0) == image_words(model, blob3, 1)
    hd = codec._parse(blob)
    K0 = ec.StepGrid.from_header(hd).indexes(h, w)
    M = 24 * int(ec.count_runs(K0)[0]) if kind == "map" else 0
    slack = 16 * (hd["sz"] * hd["lz"] + hd["sy"] * hd["ly"])
    top = 32 - int(K0.min())
    files = [model.transcode(blob, shift=d) for d in range(top + 1)]
    file_bits = [8 * len(f) for f in files]
    pay = []
    for f in files:
        fh = codec._parse(f)
        pay.append(16 * (fh["zw"] + fh["yw"]))
    print(f"\n{kind}: file bits by shift {file_bits}, M {M}, slack {slack}")
    budget_of = lambda d: max(file_bits[d], pay[d] + M + slack) + 1
    clear = [d for d in range(1, top + 1) if all(min(file_bits[e], pay[e] + M - slack) > budget_of(d) for e in range(d))]
    assert len(clear) >= 3, "fewer than three shifts whose neighbours lie further apart than the uncounted bits"
    for dstar in (clear[0], clear[len(clear) // 2], clear[-1]):
        budget = budget_of(dstar)
        want = min(d for d in range(top + 1) if file_bits[d] <= budget)                          # the rule, on the files written
        assert want == dstar
        out = model.transcode(blob, target_bpp=budget / float(H * W))
        rep = model.last_compress_report
        print(f"budget {budget}: shift {rep[0]['step_chosen']}, predicted {rep[0]['bits_predicted']:.1f}, file {8 * len(out)} bits")
        assert len(rep) == 1 and rep[0]["step_chosen"] == want and rep[0]["met"] is True and abs(rep[0]["budget_bits"] - budget) < 1e-6
        assert out == files[want] and 8 * len(out) <= budget
        assert abs(rep[0]["bits_predicted"] - (pay[want] + M)) <= slack
        assert rep[0].get("map_bits") == (float(M) if kind == "map" else None)
    # the batch: one budget per image; image 1 gets the shift it gets alone, a budget nothing exceeds keeps the file as it is
    per = [10.0 ** 9, budget_of(clear[-1]), 10.0 ** 9]
    out = model.transcode(blob3, target_bpp=[b / float(H * W) for b in per])
    rep = model.last_compress_report
    assert [r["step_chosen"] for r in rep] == [0, clear[-1], 0] and all(r["met"] for r in rep)
    assert out == model.transcode(blob3, shift=[0, clear[-1], 0])
    # a budget nothing meets: the top shift (every position at STEP_MAX), reported as not met, and the file is that shift's
    out = model.transcode(blob, target_bpp=0.25 * min(file_bits) / float(H * W))
    rep = model.last_compress_report
    assert rep[0]["step_chosen"] == top and rep[0]["met"] is False
    assert out == files[top] and codec._parse(out)["steps"] == [32]
    # several blobs: one report per blob
    many = model.transcode_many([blob, blob3], target_bpp=[budget_of(clear[0]) / float(H * W), 10.0 ** 9 / float(H * W)])
    assert [len(r) for r in model.last_compress_report] == [1, 3]
    assert many[0] == files[clear[0]] and many[1] == model.transcode(blob3, shift=0)


def test_corrupt_sources_yield_no_file(dev, hyper_model):
    from shallow_ntc_amd import _capi as capi
    model = hyper_model
    H, W = SIZES[1]
    good = source_file(model, "unit", H, W, dev)["blob"]
    src = source_file(model, "map", H, W, dev)["blob"]
    hd = model._get_codec()._parse(src)
    assert hd["zw"] > 8 and hd["yw"] > 64
    for word in (hd["pos"] // 2 + hd["zw"] // 2, hd["pos"] // 2 + hd["zw"] + hd["yw"] // 2):     # in the z streams, in the y streams
        raw = bytearray(src)
        raw[2 * word] ^= 0x10
        for call in (lambda b: model.transcode(b, shift=2), lambda b: model.transcode(b, target_bpp=0.5),
                     lambda b: model.transcode_many([good, b], shift=2)):
            with pytest.raises(capi.SntcError, match="corrupt"):
                call(bytes(raw))
    for cut in (src[:-2], src[:40], src[:hd["pos"] - 1], src + b"\0\0", b"JUNK" + src[4:]):
        with pytest.raises(capi.SntcError):
            model.transcode(cut, shift=2)
        with pytest.raises(capi.SntcError):
            model.transcode_many([good, cut], target_bpp=0.5)
    forged = bytearray(src)
    forged[4] = 6
    with pytest.raises(capi.SntcError) as e:
        model.transcode(bytes(forged), shift=1)
    assert e.value.code == capi.ERR_UNSUPPORTED
    assert model.transcode(src, shift=2) == model.transcode(bytes(src), shift=2)                 # and the model still works
