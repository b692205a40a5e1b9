"""Host half of the coded pixel residual layer ("residual layer"): the guarantee of the rule, the exact table
choice, wire format 8 and every refusal that needs no device.  No GPU."""
from pathlib import Path

import numpy as np
import pytest

import residual_cases as rc
from test_quant_step_host import header_case, shapes
from test_transcode_host import fields, i8

GOLDEN = Path(__file__).resolve().parent / "golden" / "bitstream.npz"


def test_guarantee_for_every_pixel_base_and_bound():
    """|x8 - x~| <= delta for every (x8, b, delta) in 256 x 256 x {0 .. 127}; delta = 0 reproduces x8; q stays in its range."""
    x8, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for delta in range(128):
        q = rc.quantize(x8, b, delta)
        rec = rc.reconstruct(b, q, delta)
        assert int(np.abs(x8 - rec).max()) <= delta, delta
        assert int(np.abs(q).max()) <= rc.q_max(delta) <= 255, delta
        if delta == 0:
            assert (rec == x8).all() and (q == x8 - b).all()
    # the clip is needed and harmless: b + q m may leave [0, 255] only towards the side x8 is on
    assert int((b + rc.quantize(x8, b, 127) * 255).max()) > 255


def test_classes_on_a_hand_made_picture():
    base = np.zeros((1, 3, 4, 1), np.uint8)
    base[0, 1] = [[0], [1], [3], [255]]
    cls = rc.classes(base)[0, :, :, 0]
    # row 1: a = |b(j+1) - b(j-1)| + |0 - 0| = 1, 3, 254, 252 -> levels 1, 2, 7 (capped: floor(log2 254) + 1 = 8), 7
    assert cls[1].tolist() == [1, 2, 7, 7]
    # rows 0 and 2: the vertical pair is (row, row 1) clamped: a = b(1, j) -> 0, 1, 3, 255 -> levels 0, 1, 2, 7
    assert cls[0].tolist() == cls[2].tolist() == [0, 1, 2, 7]
    b = np.random.default_rng(1).integers(0, 256, size=(2, 1, 1, 3)).astype(np.uint8)
    assert (rc.classes(b) == np.arange(3)).all()                      # one pixel: every clamped neighbour is the pixel, a = 0
    b = np.array([10, 14], np.uint8).reshape(1, 1, 2, 1)              # two pixels: each sees the other once, a = 4 -> level 3
    assert (rc.classes(b) == 3).all() and (rc.classes(b.reshape(1, 2, 1, 1)) == 3).all()


def test_residual_choice_is_the_brute_force_argmin():
    from shallow_ntc_amd import entropy_coding as ec
    tabs = ec.normal_tables()
    assert -tabs[63][0] >= 255                                        # the widest table holds every residual without an ESCAPE
    price = rc.prices(tabs, ec.cost_table)
    assert (ec.residual_prices(tabs) == price).all()
    rng = np.random.default_rng(5)
    hist = np.zeros((2, 24, 511), np.uint32)
    hist[0, 0, 255] = 1000                                            # a single spike at q = 0
    hist[0, 1, 255 + 7] = 3                                           # a spike off the centre
    hist[0, 2, [0, 510]] = 40                                         # two-sided tails reaching +-255: ESCAPE under narrow tables
    hist[0, 2, 250:261] = 500
    hist[0, 3] = rng.integers(0, 50, size=511)                        # a flat class
    hist[0, 4, 255 - 30:255 + 31] = rng.integers(0, 2000, size=61)
    hist[0, 5, 255] = 0xFFFFFFFF                                      # the largest count a bin can hold
    hist[1, 7, 100:400] = 9                                           # the other image: everything else empty
    choice, cost = ec.residual_choice(hist, tabs)
    assert choice.dtype == np.uint8 and choice.shape == (2, 24) and cost.dtype == np.int64 and cost.shape == (2,)
    total = np.zeros((2, 24, 64), dtype=object)                       # Python integers: no rounding, no overflow
    for i in range(2):
        for k in range(24):
            nz = np.flatnonzero(hist[i, k])
            for t in range(64):
                total[i, k, t] = sum(int(hist[i, k, b]) * int(price[t, b]) for b in nz)
    for i in range(2):
        want = 0
        for k in range(24):
            row = list(total[i, k])
            assert int(choice[i, k]) == row.index(min(row)), (i, k)   # list.index: the lower index on a tie
            want += min(row)
        assert int(cost[i]) == want
    assert choice[0, 0] == 0 and (choice[1, :7] == 0).all() and (choice[0, 6:] == 0).all()      # empty classes take table 0
    assert choice[0, 2] > choice[0, 0]
    # the tails are priced as ESCAPEs under the table a tail-less class would take
    assert price[choice[0, 0], 0] == price[choice[0, 0], 510] > 16 * ec.COST_UNIT
    with pytest.raises(ValueError):
        ec.residual_choice(hist[:, :, :510], tabs)
    with pytest.raises(ValueError):
        ec.residual_choice(hist.astype(np.float64), tabs)


def bases(n, H, W):
    """A v3, a v5 and a v7 blob of one header case."""
    from shallow_ntc_amd import entropy_coding as ec
    case, payload = header_case(n, H, W)
    h, w = case["dims"][4:]
    kmap = i8(np.random.default_rng(H).integers(-4, 5, size=(n, h, w)))
    kmap[:, 0, :2] = (-32, 24)
    grids = [ec.StepGrid("unit", n), ec.StepGrid.image([-3, 0, 4][:n] if n > 1 else [2]), ec.StepGrid("map", n, kmap=kmap)]
    blobs = [g.pack(*fields(case)) + payload for g in grids]
    assert [b[4] for b in blobs] == [3, 5, 7]
    return blobs


def layer(ec, base, max_error, rng, words=None):
    _, _, n, H, W = ec._base_dims(base)
    segments, lanes = ec.residual_streams(H, W)
    choice = rng.integers(0, 64, size=(n, 24)).astype(np.uint8)
    lens = rng.integers(2 * lanes, 2 * lanes + 40, size=n * segments)
    if words is None:
        words = rng.integers(0, 65536, size=int(lens.sum())).astype("<u2")
    return ec.pack_v8(0, max_error, base, segments, lanes, choice, lens) + words[:int(lens.sum())].tobytes(), choice, lens, (segments, lanes)


@pytest.mark.parametrize("n,H,W", [(1, 64, 64), (3, 200, 120), (2, 512, 768)])
def test_v8_round_trips_over_v3_v5_v7(n, H, W):
    from shallow_ntc_amd import entropy_coding as ec
    rng = np.random.default_rng(n * H)
    gold = np.load(GOLDEN)
    coded = np.concatenate([gold["words_s3"], gold["words_s1"]] * 40).astype("<u2")      # a real coder's words as the payload
    assert ec.residual_streams(512, 768) == (18, 64) and ec.residual_streams(64, 64) == (1, 32) and ec.residual_streams(1, 1) == (1, 8)
    for base in bases(n, H, W):
        for max_error in (0, 1, 127):
            blob, choice, lens, (segments, lanes) = layer(ec, base, max_error, rng, coded)
            assert blob[:4] == b"SNTC" and blob[4] == 8 and blob[5] == 0 and ec.is_residual(blob) and not ec.is_residual(base)
            back, info = ec.split_residual(blob)
            assert back == base
            assert (info["max_error"], info["n"], info["H"], info["W"], info["segments"], info["lanes"]) == (max_error, n, H, W, segments, lanes)
            assert (info["choice"] == choice).all() and info["lens"].tolist() == lens.tolist() and info["arith"] == 0
            assert blob[info["pos"]:] == coded[:int(lens.sum())].tobytes() and info["words"] == int(lens.sum())
            back, hd, info2 = ec.parse_v8(blob, "fp32", shapes)
            assert back == base and (hd["n"], hd["H"], hd["W"]) == (n, H, W) and info2["pos"] == info["pos"]
            assert ec.StepGrid.from_header(hd).kind == {3: "unit", 5: "image", 7: "map"}[base[4]]


def test_v8_refusals():
    from shallow_ntc_amd import entropy_coding as ec
    rng = np.random.default_rng(3)
    v3, v5, v7 = bases(3, 200, 120)
    blob, choice, lens, (segments, lanes) = layer(ec, v5, 2, rng)
    base_at = 4 + 8
    tail_at = base_at + len(v5)
    err = ec.capi.SntcError

    def patched(at, value):
        b = bytearray(blob)
        b[at:at + len(value)] = value
        return bytes(b)

    ec.split_residual(blob)
    with pytest.raises(err, match="truncated"):
        ec.split_residual(blob[:-1])
    with pytest.raises(err, match="does not announce"):
        ec.split_residual(blob + b"\0")
    for cut in (3, 8, 11, base_at + 10, tail_at + 2, tail_at + 4 + 10, len(blob) - lens[-1] * 2 - 2):
        with pytest.raises(err):
            ec.split_residual(blob[:cut])
    with pytest.raises(err, match="not an SNTC"):
        ec.split_residual(b"SNTX" + blob[4:])
    with pytest.raises(err, match="version 5"):
        ec.split_residual(v5)
    with pytest.raises(err, match="max_error 128"):
        ec.split_residual(patched(6, b"\x80"))
    with pytest.raises(err, match="levels"):
        ec.split_residual(patched(7, b"\x07"))
    with pytest.raises(err, match="names table 64"):
        ec.split_residual(patched(tail_at + 4 + 5, b"\x40"))
    with pytest.raises(err, match="version 8 base"):                  # a nested layer
        ec.split_residual(patched(base_at + 4, b"\x08"))
    with pytest.raises(err, match="version 4 base"):                  # a factorized-prior file
        ec.split_residual(patched(base_at + 4, b"\x04"))
    with pytest.raises(err, match="arithmetics"):
        ec.split_residual(patched(5, b"\x01"))
    for at, value in ((tail_at, b"\x09\x00"), (tail_at + 2, b"\x20"), (tail_at + 3, b"\x01")):    # segments, lanes, the zero byte
        with pytest.raises(err, match="segment / lane"):
            ec.split_residual(patched(at, value))
    with pytest.raises(err, match="truncated"):                       # a base_len that runs past the blob
        ec.split_residual(patched(8, (len(blob)).to_bytes(4, "little")))
    with pytest.raises(err):                                          # a base_len that cuts the base short: the tail no longer fits
        ec.split_residual(patched(8, (len(v5) - 2).to_bytes(4, "little")))
    with pytest.raises(err, match="implausible"):                     # n = 0 in the base header
        ec.split_residual(patched(base_at + 6, b"\0\0"))
    with pytest.raises(err):                                          # a length field that announces more words than the blob has
        ec.split_residual(patched(tail_at + 4 + 72, b"\xff\xff\xff\x7f"))
    # the base's own checks are its decoder's: a header of another model's latents is refused by parse_v8, not by the split
    other = lambda H, W: (192,) + tuple(shapes(H, W)[1:])
    with pytest.raises(err, match="does not match"):
        ec.parse_v8(blob, "fp32", other)
    with pytest.raises(err, match="bf16x3"):
        ec.parse_v8(blob, "bf16x3", shapes)
    # the writer refuses what the reader would
    for kw in (dict(max_error=128), dict(max_error=-1), dict(max_error=True), dict(max_error=1.0), dict(base=blob), dict(base=b"SNTC"),
               dict(choice=choice[:2]), dict(choice=choice.astype(np.int64)), dict(choice=np.full_like(choice, 64)), dict(segments=segments + 1),
               dict(lanes=8), dict(lens=lens[:-1]), dict(arith=1)):
        a = dict(arith=0, max_error=2, base=v5, segments=segments, lanes=lanes, choice=choice, lens=lens)
        a.update(kw)
        with pytest.raises(ValueError):
            ec.pack_v8(a["arith"], a["max_error"], a["base"], a["segments"], a["lanes"], a["choice"], a["lens"])


class Launched(Exception):
    pass


def stand_in(**over):
    """What the residual entry points read before they touch a bitstream or the device; asking for the codec raises."""
    from shallow_ntc_amd.mshyper.models import Model

    class Stub:
        _precision = "fp32"
        factorized = False
        compress = Model.compress
        add_residual = Model.add_residual
        residual_bits = Model.residual_bits
        _check_residual_arguments = Model._check_residual_arguments
        _add_residual = Model._add_residual
        _check_step_arguments = Model._check_step_arguments

        def _get_codec(self):
            raise Launched

    stub = Stub()
    for k, v in over.items():
        setattr(stub, k, v)
    return stub


def test_model_refusals_come_before_any_launch():
    x = np.zeros((1, 16, 16, 3), np.float32)
    model = stand_in()
    for d in (0, 1, 127, np.int64(5)):
        for call in (lambda: model.compress(x, max_error=d), lambda: model.add_residual(b"SNTC", x, d), lambda: model.residual_bits(x, b"SNTC", d)):
            with pytest.raises(Launched):
                call()
    with pytest.raises(Launched):
        model.residual_bits(x, b"SNTC", [0, 1, 2])
    for d in (128, -1, 1.0, "1", True, None):
        if d is not None:                                             # compress(max_error=None) is the plain file
            with pytest.raises(ValueError, match="max_error"):
                model.compress(x, max_error=d)
        with pytest.raises(ValueError, match="max_error"):
            model.add_residual(b"SNTC", x, d)
        with pytest.raises(ValueError, match="max_error"):
            model.residual_bits(x, b"SNTC", d)
    with pytest.raises(ValueError, match="max_error"):
        model.residual_bits(x, b"SNTC", [0, 128])
    for stub, word in ((stand_in(factorized=True), "hyperprior"), (stand_in(_precision="bf16x3"), "bf16x3")):
        with pytest.raises(NotImplementedError, match=word):
            stub.compress(x, max_error=1)
        with pytest.raises(NotImplementedError, match=word):
            stub.add_residual(b"SNTC", x, 1)
        with pytest.raises(NotImplementedError, match=word):
            stub.residual_bits(x, b"SNTC", 1)


def test_codec_refuses_a_layered_blob_before_any_launch():
    """``transcode`` / ``add_residual`` / ``residual_bits`` on a v8 blob: a ValueError that names the way out, raised on a codec
    made without its device tables."""
    from shallow_ntc_amd import entropy_coding as ec
    blob, *_ = layer(ec, bases(1, 64, 64)[0], 1, np.random.default_rng(0))

    class M:
        _precision = "fp32"

        def _as_device_images(self, x):
            raise Launched

    codec = ec.Codec.__new__(ec.Codec)
    codec.m = M()
    codec.latent_shapes = shapes
    x = np.zeros((1, 64, 64, 3), np.float32)
    for call in (lambda: codec.transcode(blob, shift=1), lambda: codec.transcode_many([blob], target_bpp=0.3), lambda: codec.add_residual(blob, x, 1),
                 lambda: codec.residual_bits(x, blob, [0, 1])):
        with pytest.raises(ValueError, match="split_residual"):
            call()
    with pytest.raises(ValueError, match="max_error"):
        codec.add_residual(blob, x, 128)
    codec.m._precision = "bf16x3"
    with pytest.raises(NotImplementedError, match="bf16x3"):
        codec.add_residual(ec.split_residual(blob)[0], x, 1)
