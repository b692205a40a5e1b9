"""Host half of transcoding a bitstream to a coarser quantisation step ("transcode"): the grid a file moves to
(``StepGrid.shifted``), its header, the selection over shifts and every refusal of ``Model.transcode`` -- the refusals on a stand-in
whose first device call raises (the pattern of test_sga_step_host.py).  No GPU."""
import numpy as np
import pytest

from test_quant_step_host import header_case, shapes


def i8(a):
    return np.asarray(a, np.int8)


def fields(case, arith=0):
    return (arith, case["n"], case["H"], case["W"], case["dims"], case["sz"], case["sy"], case["lz"], case["ly"], case["zl"], case["yl"])


def indexes_of(grid, h, w):
    return np.asarray(grid.indexes(h, w), np.int64)


# ------------------------------------------------------------------ the grid ------------------------------------------------
def test_check_shifts():
    from shallow_ntc_amd import entropy_coding as ec
    assert ec.check_shifts(4, 3) == [4, 4, 4] and ec.check_shifts([0, 64, 1], 3) == [0, 64, 1] and ec.check_shifts(np.int64(5), 1) == [5]
    with pytest.raises(ValueError, match="finer"):
        ec.check_shifts(-1, 2)
    with pytest.raises(ValueError, match="finer"):
        ec.check_shifts([0, -3], 2)
    for bad, n in ((65, 1), ([1, 2], 3), ([1, 2.5], 2), (1.0, 1), ("3", 1), ([True, 1], 2), (True, 1), (None, 1)):
        with pytest.raises(ValueError):
            ec.check_shifts(bad, n)


def test_shifted_unit_and_image_grids():
    from shallow_ntc_amd import entropy_coding as ec
    unit = ec.StepGrid("unit", 3)
    assert unit.shifted(0).kind == "unit" and unit.shifted([0, 0, 0]).kind == "unit"
    g = unit.shifted(5)
    assert g.kind == "image" and g.steps == [5, 5, 5] and g.n == 3
    g = unit.shifted([0, 2, 64])
    assert g.kind == "image" and g.steps == [0, 2, 32]              # clipped at STEP_MAX
    img = ec.StepGrid.image([-3, 0, 4])
    assert img.shifted(0).steps == [-3, 0, 4]
    assert img.shifted([3, 0, 1]).steps == [0, 0, 5]
    assert img.shifted(30).steps == [27, 30, 32]
    assert img.shifted(64).steps == [32, 32, 32]
    back = ec.StepGrid.image([-3, -1]).shifted([3, 1])              # every index 0: the unit grid, wire format 3
    assert back.kind == "unit" and back.n == 2 and back.steps is None
    # pure: the source is what it was
    assert img.steps == [-3, 0, 4] and unit.kind == "unit" and unit.steps is None
    for bad in (-1, [0, 0], [0, 0, -2], 65, 1.5):
        with pytest.raises(ValueError):
            img.shifted(bad)


def test_shifted_map_collapses_like_resolve():
    from shallow_ntc_amd import entropy_coding as ec
    kmap = i8([[[-32, -4, 0], [7, 30, 32]], [[1, 1, 1], [1, 2, 1]]])
    src = ec.StepGrid("map", 2, kmap=kmap)
    for d in (0, 1, [0, 5], [3, 29], [40, 0]):
        ds = ec.check_shifts(d, 2)
        want = np.clip(kmap.astype(np.int64) + np.array(ds).reshape(2, 1, 1), -32, 32)
        g = src.shifted(d)
        assert (indexes_of(g, 2, 3) == want).all(), d
        varies = any(len(np.unique(w)) > 1 for w in want)
        assert g.kind == ("map" if varies else "image"), d
        if g.kind == "map":
            assert g.kmap.dtype == np.int8 and g.kmap.shape == kmap.shape
    # map -> image: image 0 clipped flat to 32 and image 1 to 32 as well; one of them 31 keeps it an image grid, not a map
    g = src.shifted([64, 31])
    assert g.kind == "image" and g.steps == [32, 32]
    g = src.shifted([64, 30])
    assert g.kind == "map"                                          # image 1 still varies: 31 and 32
    # map -> unit needs every position at 0: only a constant map can get there
    flat = ec.StepGrid("map", 2, kmap=i8(np.full((2, 2, 3), -2)))
    assert flat.shifted(2).kind == "unit" and flat.shifted([2, 3]).steps == [0, 1]
    assert (src.kmap == kmap).all()                                  # pure


@pytest.mark.parametrize("n,H,W", [(1, 64, 64), (3, 200, 120)])
def test_shifted_headers_parse_back(n, H, W):
    """``pack`` of the shifted grid is wire format 3, 5 or 7 and parses back to the indexes clip(k + d)."""
    from shallow_ntc_amd import entropy_coding as ec
    case, payload = header_case(n, H, W)
    h, w = case["dims"][4:]
    rng = np.random.default_rng(n + H)
    kmap = i8(rng.integers(-32, 33, size=(n, h, w)) // 8 * 8)
    kmap[:, 0, :2] = (-32, 24)
    sources = [ec.StepGrid("unit", n), ec.StepGrid.image([-3, 0, 4][:n]), ec.StepGrid("map", n, kmap=kmap)]
    for src in sources:
        k0 = indexes_of(src, h, w)
        for d in (0, 3, [1, 0, 7][:n], 64):
            ds = np.array(ec.check_shifts(d, n)).reshape(n, 1, 1)
            want = np.clip(k0 + ds, -32, 32)
            g = src.shifted(d)
            blob = g.pack(*fields(case)) + payload
            constant = all(len(np.unique(x)) == 1 for x in want)
            version = 7 if not constant else 5 if want.any() else 3
            assert blob[4] == version == {"unit": 3, "image": 5, "map": 7}[g.kind], (src.kind, d)
            hd = (ec.parse_v7 if version == 7 else ec.parse_v3)(blob, "fp32", shapes)
            back = ec.StepGrid.from_header(hd)
            assert back.kind == g.kind and (indexes_of(back, h, w) == want).all(), (src.kind, d)
            assert hd["zl"].tolist() == case["zl"].tolist() and hd["yl"].tolist() == case["yl"].tolist()


# ------------------------------------------------------------------ selection -----------------------------------------------
def test_selection_over_shifts_with_map_bits():
    """``select_steps`` with the shifts d = 0 .. D as its steps: the smallest d that fits after the map's bits are added."""
    from shallow_ntc_amd import entropy_coding as ec
    shifts = list(range(0, 41))
    mono = np.array([4000.0 * 0.9 ** d for d in shifts])
    wavy = mono.copy()
    wavy[7] = mono[2] + 1.0                                          # a row need not be monotone
    bits = np.stack([mono, mono, wavy, mono])
    map_bits = np.array([0.0, 240.0, 48.0, 24.0])
    budgets = [0.5 * (mono[5] + mono[4]),                            # no map bits: 5
               0.5 * (mono[5] + mono[4]),                            # 240 bits of map push the same budget to a larger shift
               mono[2] + 48.0,                                       # exactly bits(2) + map: fits at 2 although 7 costs more
               10.0]                                                 # nothing fits
    rep = ec.select_steps(bits, budgets, shifts, map_bits)
    assert rep[0]["step_chosen"] == 5 and rep[0]["map_bits"] == 0.0
    want1 = min(d for d in shifts if mono[d] + 240.0 <= budgets[1])
    assert rep[1]["step_chosen"] == want1 > 5 and rep[1]["bits_predicted"] == mono[want1] + 240.0
    assert rep[2]["step_chosen"] == 2 and rep[2]["bits_predicted"] == budgets[2]
    assert all(r["met"] for r in rep[:3]) and rep[3]["met"] is False
    for r, row, m, b in zip(rep[:3], bits, map_bits, budgets):
        assert all(row[d] + m > b for d in shifts if d < r["step_chosen"])          # nothing smaller fits


# ------------------------------------------------------------------ refusals ------------------------------------------------
class Launched(Exception):
    pass


def stand_in(**over):
    """What ``transcode`` reads before it touches a bitstream or the device; asking for the codec raises."""
    from shallow_ntc_amd.mshyper.models import Model

    class Stub:
        _precision = "fp32"
        factorized = False
        transcode = Model.transcode
        transcode_many = Model.transcode_many
        _check_transcode_arguments = Model._check_transcode_arguments

        def _get_codec(self):
            raise Launched

    stub = Stub()
    for k, v in over.items():
        setattr(stub, k, v)
    return stub


BLOB = b"SNTC" + bytes(64)


def test_transcode_refusals_come_before_any_launch():
    model = stand_in()
    for kw in (dict(shift=0), dict(shift=3), dict(shift=[1, 2]), dict(shift=np.int64(64)), dict(target_bpp=0.3), dict(target_bpp=[0.3, 0.4])):
        with pytest.raises(Launched):                              # the stand-in works: a valid call reaches the codec
            model.transcode(BLOB, **kw)
        with pytest.raises(Launched):
            model.transcode_many([BLOB, BLOB], **kw)
    with pytest.raises(Launched):
        model.transcode_many([BLOB, BLOB], shift=[[1, 2], 3])
    for call in (lambda **kw: model.transcode(BLOB, **kw), lambda **kw: model.transcode_many([BLOB], **kw)):
        with pytest.raises(ValueError, match="exactly one"):
            call()
        with pytest.raises(ValueError, match="exactly one"):
            call(shift=1, target_bpp=0.3)
        for bad in (-1, [0, -2], [[1, -1], 0]):
            with pytest.raises(ValueError, match="finer"):
                call(shift=bad)
        for bad in (65, 1.5, "2", [1, 2.0], True, [[1, None]]):
            with pytest.raises(ValueError):
                call(shift=bad)
    fact = stand_in(factorized=True)
    split = stand_in(_precision="bf16x3")
    for kw in (dict(shift=1), dict(target_bpp=0.3)):
        with pytest.raises(NotImplementedError, match="hyperprior"):
            fact.transcode(BLOB, **kw)
        with pytest.raises(NotImplementedError, match="hyperprior"):
            fact.transcode_many([BLOB], **kw)
        with pytest.raises(NotImplementedError, match="bf16x3"):
            split.transcode(BLOB, **kw)
        with pytest.raises(NotImplementedError, match="bf16x3"):
            split.transcode_many([BLOB], **kw)


def test_codec_refuses_what_needs_the_header():
    """The per-image counts are known once the header is parsed: still host work, before any launch (a codec made without its
    device tables: ``transcode_many`` reads only the model's precision and latent shapes up to there)."""
    from shallow_ntc_amd import entropy_coding as ec
    case, payload = header_case(3, 200, 120)
    blob = ec.StepGrid.image([1, 0, 2]).pack(*fields(case)) + payload

    class M:
        _precision = "fp32"

    codec = ec.Codec.__new__(ec.Codec)
    codec.m = M()
    codec.latent_shapes = shapes
    for kw in (dict(shift=[[1, 2]]), dict(shift=[[1, 2, 3, 4]]), dict(shift=[1, 2]), dict(target_bpp=[[0.3, 0.4]]), dict(target_bpp=[0.1, 0.2])):
        with pytest.raises(ValueError):
            codec.transcode_many([blob], **kw)
    with pytest.raises(ValueError, match="exactly one"):
        codec.transcode_many([blob])
    codec.m._precision = "bf16x3"
    with pytest.raises(NotImplementedError, match="bf16x3"):
        codec.transcode_many([blob], shift=1)
    codec.m._precision = "fp32"
    with pytest.raises(ec.capi.SntcError, match="truncated"):
        codec.transcode_many([blob[:-2]], shift=1)
    assert codec.transcode_many([], shift=1) == []
