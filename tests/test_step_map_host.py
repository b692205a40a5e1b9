"""Host half of region-of-interest coding ("variable rate"): per-position offsets on the quantisation-step ladder,
their run-length records, wire format v7 (the v3 header + the records), the mask helper and the rate-control rule with the map's
bits are pure functions.  No GPU."""
import struct

import numpy as np
import pytest

from test_quant_step_host import header_case, pack, shapes


def i8(a):
    return np.asarray(a, np.int8)


def records(buf):
    return [struct.unpack_from("<bH", buf, o) for o in range(0, len(buf), 3)]


# ------------------------------------------------------------------ runs ---------------------------------------------------
def test_runs_round_trip():
    from shallow_ntc_amd import entropy_coding as ec
    rng = np.random.default_rng(0)
    cases = {
        "constant": (np.full((2, 40), -7), [(-7, 40), (-7, 40)]),
        "alternating": (np.tile([3, -3], (1, 5)), [(3, 1), (-3, 1)] * 5),
        "one position": (np.array([[32], [-32], [0]]), [(32, 1), (-32, 1), (0, 1)]),
        "long run": (np.concatenate([np.full(65536 + 1, 5), [6]])[None], [(5, 65535), (5, 2), (6, 1)]),
        "two full records": (np.full((1, 2 * 65535), 1), [(1, 65535), (1, 65535)]),
        # equal values on both sides of both image boundaries: the runs must not merge
        "image boundary": (np.array([[1, 1, 2, 2], [2, 2, 2, 3], [3, 0, 0, 0]]), [(1, 2), (2, 2), (2, 3), (3, 1), (3, 1), (0, 3)]),
        "random": (rng.integers(-32, 33, size=(3, 257)), None),
    }
    for name, (K, want) in cases.items():
        K = i8(K)
        buf = ec.pack_runs(K)
        assert len(buf) % 3 == 0, name
        got = records(buf)
        if want is not None:
            assert got == want, name
        assert all(1 <= r <= 65535 for _, r in got), name
        back = ec.parse_runs(buf, *K.shape)
        assert back.dtype == np.int8 and back.shape == K.shape and (back == K).all(), name
        # maximal: two neighbouring records of one image differ in value, unless the first is a full one
        pos = 0
        for (ka, ra), (kb, _) in zip(got, got[1:]):
            pos += ra
            assert ka != kb or ra == 65535 or pos % K.shape[1] == 0, name
    for bad in (np.zeros((2, 3), np.int16), np.zeros(6, np.int8), i8([[33, 0]]), i8([[0, -33]])):
        with pytest.raises(ValueError):
            ec.pack_runs(bad)


def test_parse_runs_refusals():
    from shallow_ntc_amd import entropy_coding as ec
    rec = lambda *pairs: b"".join(struct.pack("<bH", k, r) for k, r in pairs)
    n, hw = 2, 6
    assert ec.parse_runs(rec((1, 6), (2, 2), (1, 4)), n, hw).tolist() == [[1] * 6, [2, 2, 1, 1, 1, 1]]
    for what, buf in (("index", rec((33, 6), (0, 6))), ("index", rec((1, 6), (-33, 6))), ("length 0", rec((1, 6), (2, 0), (2, 6))),
                      ("crosses", rec((1, 5), (2, 2), (1, 5))), ("crosses", rec((1, 12))), ("covers", rec((1, 6), (2, 5))),
                      ("covers", rec((1, 6), (2, 6), (2, 1))), ("covers", b""), ("whole number", rec((1, 6), (2, 6))[:-1])):
        with pytest.raises(ec.capi.SntcError, match=what) as e:
            ec.parse_runs(buf, n, hw)
        assert e.value.code == ec.capi.ERR_BAD_SHAPE


# ------------------------------------------------------------------ wire format 7 ------------------------------------------
def map_case(n, H, W, seed=0):
    case, payload = header_case(n, H, W)
    h, w = case["dims"][4:]
    rng = np.random.default_rng(seed)
    kmap = i8(rng.integers(-32, 33, size=(n, h, w)) // 8 * 8)
    kmap[:, 0, :2] = (-32, 32)                          # every image varies, both ends of the ladder present
    return case, payload, kmap


def pack7(case, kmap, arith=0):
    from shallow_ntc_amd import entropy_coding as ec
    return ec.pack_v7(arith, case["n"], case["H"], case["W"], case["dims"], case["sz"], case["sy"], case["lz"], case["ly"], case["zl"],
                      case["yl"], kmap)


@pytest.mark.parametrize("n", [1, 3])
def test_v7_layout(n):
    from shallow_ntc_amd import entropy_coding as ec
    case, payload, kmap = map_case(n, 200, 120)
    c, cz, hz, wz, h, w = case["dims"]
    recs = ec.pack_runs(kmap.reshape(n, -1))
    for arith, prec in ((0, "fp32"), (1, "bf16x3")):
        blob = pack7(case, kmap, arith) + payload
        want = b"SNTC" + struct.pack("<HHIIHHHHHHHHBB", 7 | (arith << 8), n, 200, 120, c, cz, hz, wz, h, w, case["sz"], case["sy"],
                                     case["lz"], case["ly"])
        want += struct.pack("<I", len(recs) // 3) + recs
        want += b"".join(struct.pack("<I", int(v)) for v in case["zl"]) + b"".join(struct.pack("<I", int(v)) for v in case["yl"])
        assert blob == want + payload and blob[4] == ec.VERSION_MAP == 7 and blob[5] == arith
        hd = ec.parse_v7(blob, prec, shapes)
        assert hd["steps"] is None and hd["kmap"].dtype == np.int8 and hd["kmap"].shape == (n, h, w) and (hd["kmap"] == kmap).all()
        assert hd["pos"] == len(want) == len(blob) - len(payload)
        # everything else is the parse_v3 dict of the same fields
        v3 = ec.parse_v3(pack(case, None, arith) + payload, prec, shapes)
        assert set(hd) == set(v3) | {"kmap"}
        for key in set(v3) - {"pos", "steps", "zl", "yl"}:
            assert hd[key] == v3[key], key
        assert hd["zl"].tolist() == v3["zl"].tolist() and hd["yl"].tolist() == v3["yl"].tolist()
        with pytest.raises(ec.capi.SntcError) as e:          # the other arithmetic: refused as parse_v3 refuses it
            ec.parse_v7(blob, "bf16x3" if prec == "fp32" else "fp32", shapes)
        assert e.value.code == ec.capi.ERR_UNSUPPORTED


def test_writer_is_canonical():
    """Constant maps are the v5 bytes of pack_v3 (v3 where every index is 0): version 7 only for a map that really varies."""
    from shallow_ntc_amd import entropy_coding as ec
    case, payload = header_case(3, 128, 128)
    h, w = case["dims"][4:]
    full = lambda ks: i8(np.broadcast_to(np.reshape(ks, (3, 1, 1)), (3, h, w)))
    assert pack7(case, full([3, -2, 32])) == pack(case, [3, -2, 32]) and pack(case, [3, -2, 32])[4] == 5
    assert pack7(case, full([0, 5, 0])) == pack(case, [0, 5, 0])
    assert pack7(case, full([0, 0, 0])) == pack(case, None) and pack(case, None)[4] == 3
    one = full([0, 0, 0]).copy()
    one[1, h - 1, w - 1] = 1                             # one position of one image differs
    blob = pack7(case, one)
    assert blob[4] == 7 and (ec.parse_v7(blob + payload, "fp32", shapes)["kmap"] == one).all()
    for bad in (full([0, 0, 0])[:2], full([0, 0, 0]).astype(np.int16), full([0, 0, 33]), full([0, 0, 0])[:, :-1]):
        with pytest.raises(ValueError):
            pack7(case, bad)


def test_v7_refusals():
    from shallow_ntc_amd import entropy_coding as ec
    case, payload, kmap = map_case(3, 200, 120)
    n, (h, w) = 3, case["dims"][4:]
    blob = pack7(case, kmap) + payload
    fixed = 4 + struct.calcsize(ec.HEAD_V3)
    count = struct.unpack_from("<I", blob, fixed)[0]
    first = fixed + 4

    def refused(b, match, code=ec.capi.ERR_BAD_SHAPE):
        with pytest.raises(ec.capi.SntcError, match=match) as e:
            ec.parse_v7(bytes(b), "fp32", shapes)
        assert e.value.code == code

    def patched(offset, fmt, *values):
        b = bytearray(blob)
        struct.pack_into(fmt, b, offset, *values)
        return b

    recs = records(blob[first:first + 3 * count])
    n0 = len(ec.pack_runs(kmap[:1].reshape(1, -1))) // 3               # records of image 0
    assert recs[n0] == (-32, 1) and sum(r for _, r in recs[:n0]) == h * w

    def with_records(rs):
        return blob[:fixed] + struct.pack("<I", len(rs)) + b"".join(struct.pack("<bH", k, r) for k, r in rs) + blob[first + 3 * count:]

    assert ec.parse_v7(with_records(recs), "fp32", shapes)["kmap"].tolist() == kmap.tolist()
    for forged in (33, -33, 127, -128):
        refused(patched(first, "<b", forged), "index")
        refused(patched(first + 3 * (count - 1), "<b", forged), "index")
    refused(with_records(recs[:1] + [(5, 0)] + recs[1:]), "length 0")
    refused(with_records(recs + [(5, 1)]), "covers")                      # one position too many in all
    refused(with_records(recs[:-1]), "covers")                            # the last run missing
    # image 0's last run takes image 1's first position: n h w in all, but no record ends where image 0 does
    refused(with_records(recs[:n0 - 1] + [(recs[n0 - 1][0], recs[n0 - 1][1] + 1)] + recs[n0 + 1:]), "crosses")
    assert n * h * w <= 65535
    refused(with_records([(4, n * h * w)]), "crosses")                    # one run over all three images
    refused(patched(fixed, "<I", n * h * w + 1), "records")                # a record count above n h w
    refused(patched(fixed, "<I", count + 1), "truncated|covers|index|crosses|length 0")     # the length fields read as a record
    lens_end = first + 3 * count + 4 * n * (case["sz"] + case["sy"])
    for cut in (fixed - 1, fixed, fixed + 3, first, first + 2, first + 3 * count - 1, lens_end - 1, len(blob) - 2, len(blob) - 1):
        refused(blob[:cut], "truncated")
    refused(blob + b"\0\0", "truncated")
    for ver in (2, 3, 4, 5, 6):                                           # parse_v7 reads version 7 alone
        refused(patched(4, "<B", ver), "version", ec.capi.ERR_UNSUPPORTED)
    refused(patched(6, "<H", 0), "implausible")                          # the header checks of parse_v3, shared
    refused(patched(8, "<I", 216), "does not match")
    refused(b"SNTX" + blob[4:], "not an SNTC")


def test_parse_v3_still_refuses_6_and_7():
    from shallow_ntc_amd import entropy_coding as ec
    case, payload, kmap = map_case(3, 200, 120)
    v5, v7 = pack(case, [3, -2, 32]) + payload, pack7(case, kmap) + payload
    for blob in (v5, v7):
        for ver in (6, 7):
            b = bytearray(blob)
            b[4] = ver
            with pytest.raises(ec.capi.SntcError) as e:
                ec.parse_v3(bytes(b), "fp32", shapes)
            assert e.value.code == ec.capi.ERR_UNSUPPORTED
    b = bytearray(v7)
    b[4] = 6                                                  # version 6 is not assigned: no parser reads it
    with pytest.raises(ec.capi.SntcError) as e:
        ec.parse_v7(bytes(b), "fp32", shapes)
    assert e.value.code == ec.capi.ERR_UNSUPPORTED


# ------------------------------------------------------------------ offsets ------------------------------------------------
def test_check_offsets():
    from shallow_ntc_amd import entropy_coding as ec
    a = np.arange(24).reshape(2, 3, 4) - 10
    got = ec.check_offsets(a, 2, 3, 4)
    assert got.dtype == np.int8 and got.flags["C_CONTIGUOUS"] and (got == a).all()
    assert (ec.check_offsets(a.astype(np.int64).transpose(0, 2, 1), 2, 4, 3) == a.transpose(0, 2, 1)).all()
    assert ec.check_offsets(np.full((1, 2, 2), 64), 1, 2, 2).tolist() == [[[64, 64], [64, 64]]]
    assert ec.check_offsets(a.tolist(), 2, 3, 4).tolist() == a.tolist()
    for bad in (a[0], a[:, :2], a.reshape(2, 4, 3), a.astype(np.float32), a > 0, np.full((2, 3, 4), 65), np.full((2, 3, 4), -65),
                a.astype(np.float64).tolist(), None, "x"):
        with pytest.raises(ValueError):
            ec.check_offsets(bad, 2, 3, 4)
    K = ec.index_map([0, 30], i8([[[-64, -3, 0]], [[5, -64, 1]]]))
    assert K.dtype == np.int8 and K.tolist() == [[[-32, -3, 0]], [[32, -32, 31]]]
    assert ec.uniform_steps(K) is None and ec.uniform_steps(i8([[[4, 4]], [[-1, -1]]])) == [4, -1]
    assert ec.count_runs(i8([[[1, 1], [1, 2]], [[0, 1], [0, 1]], [[3, 3], [3, 3]]])).tolist() == [2, 4, 1]


def test_roi_offsets():
    """Hand-worked masks at 16 pixels per position."""
    from shallow_ntc_amd import entropy_coding as ec
    blank = lambda H, W: np.zeros((1, H, W), np.bool_)
    inside = lambda off: sorted(map(tuple, np.argwhere(off[0] == 0).tolist()))
    # a single pixel: position (37 // 16, 70 // 16) = (2, 4); grow = 1 its 8 neighbours too
    m = blank(96, 128)
    m[0, 37, 70] = True
    off = ec.roi_offsets(m, 16, grow=0)
    assert off.dtype == np.int8 and off.shape == (1, 6, 8) and inside(off) == [(2, 4)] and (off == 12).sum() == 47
    assert inside(ec.roi_offsets(m, 16)) == [(r, c) for r in (1, 2, 3) for c in (3, 4, 5)]
    assert inside(ec.roi_offsets(m, 16, grow=2)) == [(r, c) for r in range(0, 5) for c in range(2, 7)]
    # a block that ends ON a block edge (rows 16 .. 31, columns 32 .. 63) does not spill; one pixel more does
    m = blank(96, 128)
    m[0, 16:32, 32:64] = True
    assert inside(ec.roi_offsets(m, 16, grow=0)) == [(1, 2), (1, 3)]
    m[0, 32, 63] = True
    assert inside(ec.roi_offsets(m, 16, grow=0)) == [(1, 2), (1, 3), (2, 3)]
    # in a corner the dilation stays inside the map
    m = blank(96, 128)
    m[0, 0, 0] = True
    assert inside(ec.roi_offsets(m, 16)) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    # 200 x 120: 13 x 8 positions, the last row / column half padding; a mask on the image's last row touches them
    m = blank(200, 120)
    m[0, 199, 119] = True
    off = ec.roi_offsets(m, 16, inside=-4, outside=20, grow=0)
    assert off.shape == (1, 13, 8) and off[0, 12, 7] == -4 and (off == 20).sum() == 13 * 8 - 1
    # ... and on the latents of a model that pads to 64 (16 x 8 positions): the same position, rows 13 .. 15 all padding
    off = ec.roi_offsets(m, 16, grow=1, latent_hw=(16, 8))
    assert off.shape == (1, 16, 8) and inside(off) == [(r, c) for r in (11, 12, 13) for c in (6, 7)]
    m[0, 199, 119] = False
    assert (ec.roi_offsets(m, 16) == 12).all()
    # a batch: images keep their own masks
    m = np.zeros((2, 32, 32), np.bool_)
    m[1, 20, 5] = True
    assert ec.roi_offsets(m, 16, grow=0).tolist() == [[[12, 12], [12, 12]], [[12, 12], [0, 12]]]
    for kw in (dict(mask=m.astype(np.uint8)), dict(mask=m[0]), dict(factor=0), dict(grow=-1), dict(inside=65), dict(outside=1.5),
               dict(latent_hw=(1, 2))):
        with pytest.raises(ValueError):
            ec.roi_offsets(**dict(dict(mask=m, factor=16), **kw))


# ------------------------------------------------------------------ rate control -------------------------------------------
def test_selection_rule_with_map_bits():
    from shallow_ntc_amd import entropy_coding as ec
    ladder = list(range(ec.STEP_MIN, ec.STEP_MAX + 1))
    mono = np.array([100000.0 * 0.9 ** (k - ec.STEP_MIN) for k in ladder])          # falls 10 % per step
    at = lambda k: float(mono[ladder.index(k)])
    bits = np.stack([mono, mono, mono, mono])
    between = 0.5 * (at(7) + at(6))
    map_bits = [0.0, 24.0 * 40, 5.0, at(ec.STEP_MAX)]
    budgets = [between, between, at(6) + 5.0, 1.5 * at(ec.STEP_MAX)]
    rule = lambda mbs: [min([k for k in ladder if at(k) + mb <= b] or [None]) for mb, b in zip(mbs, budgets)]      # the rule, restated
    want, plain = rule(map_bits), rule([0.0] * 4)
    # a map of 40 runs moves image 1 from 7 to a coarser step; image 2's bits at 6 plus its map are exactly its budget: that fits;
    # image 3's map leaves no step within a budget that three steps meet without it
    assert want[0] == plain[0] == 7 and want[1] > 7 == plain[1] and want[2] == 6 and at(6) + 5.0 == budgets[2]
    assert want[3] is None and plain[3] == ec.STEP_MAX - 3
    rep = ec.select_steps(bits, budgets, ladder, map_bits)
    assert [r["step_chosen"] for r in rep] == want[:3] + [ec.STEP_MAX]
    assert [r["met"] for r in rep] == [True, True, True, False]
    for r, mb, b in zip(rep, map_bits, budgets):
        assert r["map_bits"] == mb and r["budget_bits"] == b and r["bits_predicted"] == at(r["step_chosen"]) + mb
    rep0 = ec.select_steps(bits, budgets, ladder)
    assert [r["step_chosen"] for r in rep0] == plain and all("map_bits" not in r for r in rep0)
    with pytest.raises(ValueError):
        ec.select_steps(bits, budgets, ladder, map_bits[:3])
    # 24 bits per record: what pack_runs writes for offsets whose clipped map keeps every run
    offs = i8([[[0, 0, 16, 16], [16, 0, 0, 0]]])
    assert ec.MAP_RECORD_BITS * ec.count_runs(offs)[0] == 8 * len(ec.pack_runs(ec.index_map([3], offs).reshape(1, -1))) == 24 * 3
    assert 8 * len(ec.pack_runs(ec.index_map([32], offs).reshape(1, -1))) == 24             # clipping merges runs: an upper bound


# ------------------------------------------------------------------ the grid -----------------------------------------------
def test_step_grid_routing_and_headers():
    """``StepGrid.resolve`` is the one routing rule: nothing or all zeros -> unit, a map constant per image -> image at those
    indexes (unit if all are 0), anything else -> map; ``pack`` / ``from_header`` keep the kind through the file.  Host only."""
    from shallow_ntc_amd import entropy_coding as ec
    G = ec.StepGrid
    n, (_, _, _, _, h, w) = 2, shapes(64, 64)
    zero, const, vary = np.zeros((n, h, w), np.int8), np.zeros((n, h, w), np.int8), np.zeros((n, h, w), np.int8)
    const[1], vary[0, 0, 0] = 5, 1
    for args in ((None, None), (0, None), ([0, 0], None), (None, zero), ([-5, 0], const + i8([5, -5]).reshape(n, 1, 1))):
        g = G.resolve(*args, n, h, w)
        assert g.kind == "unit" and g.steps is None and g.kmap is None and g.n == n, args
    for args, want in ((([3, -3], None), [3, -3]), ((7, None), [7, 7]), ((1, const), [1, 6]), ((None, const), [0, 5]), (([30, 30], const), [30, 32])):
        g = G.resolve(*args, n, h, w)
        assert g.kind == "image" and g.steps == want and g.kmap is None, args
    g = G.resolve([2, -40 + 8], vary, n, h, w)
    assert g.kind == "map" and g.steps is None and g.kmap.dtype == np.int8 and (g.kmap == ec.index_map([2, -32], vary)).all()
    assert G.image([0, 0]).kind == "image" and G.image([0, 0]).steps == [0, 0]         # what a per-image rd_lambda asks for
    for bad in (([1], None), (33, None), (1.5, None), (None, zero[:1]), (None, zero.astype(np.float32)), (None, zero + 65)):
        with pytest.raises(ValueError):
            G.resolve(*bad, n, h, w)
    # omega: the map's own weights; a unit or image grid broadcasts its indexes
    assert (g.position_weights() == ec.position_weights(g.kmap)).all()
    assert G.resolve(None, None, n).position_weights(h, w).tolist() == np.ones((n, h, w)).tolist()
    assert (G.resolve([3, -3], None, n).position_weights(h, w) == ec.position_weights(ec.index_map([3, -3], zero))).all()
    # the file keeps the kind: version byte 3 / 5 / 7, and the parsed header announces the same grid
    case, payload = header_case(n, 64, 64)
    fields = (0,) + tuple(case[k] for k in ("n", "H", "W", "dims", "sz", "sy", "lz", "ly", "zl", "yl"))
    for grid, version in ((G.resolve(None, zero, n, h, w), 3), (G.resolve(1, const, n, h, w), 5), (g, 7)):
        blob = grid.pack(*fields) + payload
        assert blob[4] == version
        assert blob == (ec.pack_v7(*fields, grid.kmap) if version == 7 else pack(case, grid.steps)) + payload
        hd = (ec.parse_v7 if version == 7 else ec.parse_v3)(blob, "fp32", shapes)
        back = G.from_header(hd)
        assert back.kind == grid.kind and back.steps == grid.steps and back.n == n
        assert (back.kmap is None) == (grid.kmap is None) and (grid.kmap is None or (back.kmap == grid.kmap).all())
