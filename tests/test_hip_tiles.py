"""Tiled files on the GPU (-m gpu): the two kernels of csrc/tiles.hip alone, exactly against the numpy restatements of
tests/tile_cases.py, then ``compress(x, tile=...)`` / ``decompress`` / ``decompress(region=...)`` / ``select_images`` end to end."""
import numpy as np
import pytest
import torch

import tile_cases
from test_hip_itinf_bitstream import fact_model, hyper_model, images  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

T = 8
SHAPES = [(15, 16), (17, 23), (33, 9)]


def dv(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def windows(H, W, O):
    """The whole picture, one pixel, a window that starts and ends inside bands (where the picture has any), one touching the
    last row and column."""
    def span(L):
        if L < 2 * T:                                     # one tile: no band
            return 1, min(2, L - 1)
        a = T - O + (1 if O > 1 else 0)                   # inside the first band [T - O, T + O)
        b = (2 * T if L >= 3 * T else T) + max(O - 1, 1)  # ends inside the second band where there is one, else the first
        return a, b - a

    (y0, h), (x0, w) = span(H), span(W)
    return [None, (H // 2, W // 2, 1, 1), (H - 3, W - 2, 3, 2), (y0, x0, h, w)]


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("O", [0, 1, 2])
@pytest.mark.parametrize("H,W", SHAPES)
def test_extract_is_slicing(H, W, O, c, dev):
    from shallow_ntc_amd import ops, tiling
    rng = np.random.default_rng(H * 100 + W + O)
    x = rng.standard_normal((2, H, W, c)).astype(np.float32)
    xd = dv(x, dev)
    g, plan, _ = tiling.tile_plan(2, H, W, T, O)
    want = tile_cases.extract(x, T, O)
    for b in plan:
        rects = [(i, g["rows"][r][2], g["cols"][q][2]) for i, r, q in b["tiles"]]
        got = ops.tiles_extract(xd, rects, b["th"], b["tw"]).cpu().numpy()
        for k, (i, r, q) in enumerate(b["tiles"]):
            np.testing.assert_array_equal(got[k], want[(i * g["R"] + r) * g["C"] + q])


def test_extract_vector_path_and_refusals(dev):
    """Rows of both sides 16-byte aligned (c = 4, x0 c % 4 == 0): the float4 path, the same values; a view 4 bytes into its
    allocation takes the dword path again.  A rect that leaves the image is refused before any launch."""
    from shallow_ntc_amd import _capi as capi
    from shallow_ntc_amd import ops
    rng = np.random.default_rng(5)
    x = rng.standard_normal((2, 21, 16, 4)).astype(np.float32)
    xd = dv(x, dev)
    rects = [(1, 3, 5), (0, 0, 0), (1, 11, 8)]
    want = np.stack([x[i, y:y + 10, a:a + 8] for i, y, a in rects])
    np.testing.assert_array_equal(ops.tiles_extract(xd, rects, 10, 8).cpu().numpy(), want)
    shifted = torch.cat([torch.zeros(1, device=dev), xd.flatten()])[1:].view(2, 21, 16, 4)
    np.testing.assert_array_equal(ops.tiles_extract(shifted, rects, 10, 8).cpu().numpy(), want)
    for bad in ((2, 0, 0), (0, 12, 0), (0, 0, 9), (-1, 0, 0), (0, -1, 0)):
        with pytest.raises(capi.SntcError, match="leaves the image"):
            ops.tiles_extract(xd, [(0, 0, 0), bad], 10, 8)


def decoded_tiles(H, W, O, c, dev, seed):
    rng = np.random.default_rng(seed)
    shapes = [(y1 - y0, x1 - x0) for _ in range(2) for y0, y1 in tile_cases.extents(H, T, O) for x0, x1 in tile_cases.extents(W, T, O)]
    host = [rng.integers(0, 256, (th, tw, c), dtype=np.uint8) for th, tw in shapes]
    for k in (0, len(host) - 1):                          # the extremes, where a rounding slip would show
        host[k][...] = 255 if k else 0
    return host, [dv(t, dev) for t in host]


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("O", [0, 1, 2])
@pytest.mark.parametrize("H,W", SHAPES)
def test_assemble_is_the_integer_blend(H, W, O, c, dev):
    from shallow_ntc_amd import ops
    host, tiles = decoded_tiles(H, W, O, c, dev, H + W + O + c)
    for region in windows(H, W, O):
        want, lost = tile_cases.assemble(host, 2, H, W, c, T, O, region)
        assert lost == 0
        got = ops.tiles_assemble(tiles, 2, H, W, c, T, O, region)
        np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f"region {region}")
        # an output that starts one byte into its allocation: the head and tail bytes of the unaligned store path
        h, w = want.shape[1:3]
        buf = torch.full((2 * h * w * c + 9,), 0xAB, dtype=torch.uint8, device=dev)
        out = buf[1:1 + 2 * h * w * c].view(2, h, w, c)
        assert out.data_ptr() % 4 == 1
        ops.tiles_assemble(tiles, 2, H, W, c, T, O, region, out=out)
        np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg=f"region {region}, offset base")
        edge = buf.cpu().numpy()
        assert edge[0] == 0xAB and (edge[1 + 2 * h * w * c:] == 0xAB).all()           # nothing written around it


@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_assemble_wide_units(c, dev):
    """Tiles wider than any store unit, at every channel count: long runs inside one tile column, outside and inside a ROW band,
    next to column bands and row ends; several alignments of the output base, and a missing tile.  Holds for any unit width."""
    from shallow_ntc_amd import ops
    H, W, tile, O = 70, 83, 32, 5
    rng = np.random.default_rng(c)
    host = [rng.integers(0, 256, (y1 - y0, x1 - x0, c), dtype=np.uint8)
            for _ in range(2) for y0, y1 in tile_cases.extents(H, tile, O) for x0, x1 in tile_cases.extents(W, tile, O)]
    tiles = [dv(t, dev) for t in host]
    for region in (None, (25, 3, 9, 77), (0, 40, 70, 43)):
        want, lost = tile_cases.assemble(host, 2, H, W, c, tile, O, region)
        assert lost == 0
        h, w = want.shape[1:3]
        for shift in (0, 1, 7, 15):
            buf = torch.full((2 * h * w * c + 32,), 0xAB, dtype=torch.uint8, device=dev)
            out = buf[shift:shift + 2 * h * w * c].view(2, h, w, c)
            ops.tiles_assemble(tiles, 2, H, W, c, tile, O, region, out=out)
            np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg=f"region {region}, base + {shift}")
            edge = buf.cpu().numpy()
            assert (edge[:shift] == 0xAB).all() and (edge[shift + 2 * h * w * c:] == 0xAB).all()
    # a missing tile on the 16-byte path: its pixels are 0 and counted once each
    gone, hgone = list(tiles), list(host)
    gone[1], hgone[1] = None, None                         # image 0, tile (0, 1): rows 0 .. 36, columns 27 .. 82
    out, missing = ops.tiles_assemble(gone, 2, H, W, c, tile, O, check=False)
    want, lost = tile_cases.assemble(hgone, 2, H, W, c, tile, O)
    assert lost == 37 * 56 and int(missing.item()) == lost
    np.testing.assert_array_equal(out.cpu().numpy(), want)


def test_assemble_missing_tiles(dev):
    from shallow_ntc_amd import _capi as capi
    from shallow_ntc_amd import ops
    H, W, O, c = 17, 23, 2, 3
    host, tiles = decoded_tiles(H, W, O, c, dev, 3)
    R, C = 2, 2
    assert len(tiles) == 2 * R * C
    gone = list(tiles)
    gone[1 * R * C + 1 * C + 1] = None                   # image 1, tile (1, 1): extent rows 6 .., columns 6 ..
    hgone = list(host)
    hgone[1 * R * C + 1 * C + 1] = None
    # a window that needs it: the wrapper raises; the raw call counts the pixels and writes them as 0
    with pytest.raises(capi.SntcError, match="need a tile that was not decoded"):
        ops.tiles_assemble(gone, 2, H, W, c, T, O)
    out, missing = ops.tiles_assemble(gone, 2, H, W, c, T, O, check=False)
    want, lost = tile_cases.assemble(hgone, 2, H, W, c, T, O)
    assert lost == (H - 6) * (W - 6) and int(missing.item()) == lost
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    # a window outside its extent: the null pointer is never read
    region = (0, 0, 6, 23)
    want, lost = tile_cases.assemble(hgone, 2, H, W, c, T, O, region)
    assert lost == 0
    np.testing.assert_array_equal(ops.tiles_assemble(gone, 2, H, W, c, T, O, region).cpu().numpy(), want)
    # the wrapper's own checks: a tile of the wrong shape, a window that leaves the picture
    wrong = list(tiles)
    wrong[0] = tiles[1]
    with pytest.raises(ValueError, match="tile 0"):
        ops.tiles_assemble(wrong, 2, H, W, c, T, O)
    with pytest.raises(ValueError, match="region"):
        ops.tiles_assemble(tiles, 2, H, W, c, T, O, (0, 0, 18, 23))


# -- end to end ------------------------------------------------------------------------------------------------------------
N, HH, WW, TILE = 2, 200, 150, 64


@pytest.fixture(scope="module")
def picture(dev):
    return images(N, HH, WW, dev)


def decode_tiles(model, x, O, step=None):
    """The reference of the end-to-end tests: every extent sliced with numpy, coded and decoded ON ITS OWN shape class batch by
    the untiled ``compress`` / ``decompress`` -> (the inner blobs in file order, the decoded tiles in (image, row, col) order)."""
    from shallow_ntc_amd import tiling
    xh = x.cpu().numpy()
    g, plan, _ = tiling.tile_plan(N, HH, WW, TILE, O)
    sliced = tile_cases.extract(xh, TILE, O)
    blobs, tiles = [], [None] * len(sliced)
    for b in plan:
        ids = [(i * g["R"] + r) * g["C"] + q for i, r, q in b["tiles"]]
        batch = np.stack([sliced[k] for k in ids])
        ks = None if step is None else [step[i] if isinstance(step, list) else step for i, _, _ in b["tiles"]]
        blobs.append(model.compress(batch, step=ks))
        dec = model.decompress(blobs[-1]).cpu().numpy()
        for k, t in zip(ids, dec):
            tiles[k] = t
    return blobs, tiles


@pytest.fixture(scope="module")
def tiled16(hyper_model, picture):
    blob = hyper_model.compress(picture, tile=TILE, overlap=16)
    return blob, hyper_model.decompress(blob).cpu().numpy()


def test_overlap_0_inner_blobs_are_compress_of_the_slices(hyper_model, picture):
    from shallow_ntc_amd import tiling
    blob = hyper_model.compress(picture, tile=TILE, overlap=0)
    idx = hyper_model.tile_index(blob)
    assert (idx["R"], idx["C"]) == (3, 2) and blob[4] == 9
    hd = tiling.parse_v9(blob, 0)
    want_blobs, tiles = decode_tiles(hyper_model, picture, 0)
    assert [blob[b["at"]:b["at"] + b["bytes"]] for b in hd["blobs"]] == want_blobs
    pasted = np.zeros((N, HH, WW, 3), np.uint8)
    for t, px in zip(idx["tiles"], tiles):
        pasted[t["image"], t["y0"]:t["y1"], t["x0"]:t["x1"]] = px
    got = hyper_model.decompress(blob)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (N, HH, WW, 3)
    np.testing.assert_array_equal(got.cpu().numpy(), pasted)
    assert hyper_model.last_decompress_report == dict(tiles_total=12, tiles_decoded=12, bytes_total=len(blob), bytes_read=len(blob))
    # without tile= nothing changed: the untiled file is the one an explicit step 0 / no option writes
    assert hyper_model.compress(picture)[4] == 3


def test_overlap_16_is_the_numpy_blend_of_the_decoded_extents(hyper_model, picture, tiled16):
    from shallow_ntc_amd import tiling
    blob, full = tiled16
    hd = tiling.parse_v9(blob, 0)
    want_blobs, tiles = decode_tiles(hyper_model, picture, 16)
    assert [blob[b["at"]:b["at"] + b["bytes"]] for b in hd["blobs"]] == want_blobs
    want, lost = tile_cases.assemble(tiles, N, HH, WW, 3, TILE, 16)
    assert lost == 0
    np.testing.assert_array_equal(full, want)


@pytest.mark.parametrize("region,count", [((5, 7, 30, 40), 1), ((40, 40, 60, 50), 4), ((199, 149, 1, 1), 1), ((100, 0, 100, 150), 4)],
                         ids=["one-tile", "four-tile-corner", "last-pixel", "two-rows"])
def test_region_decode_is_the_crop_of_the_full_decode(hyper_model, tiled16, region, count):
    from shallow_ntc_amd import tiling
    blob, full = tiled16
    y0, x0, h, w = region
    got = hyper_model.decompress(blob, region=region)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (N, h, w, 3)
    np.testing.assert_array_equal(got.cpu().numpy(), full[:, y0:y0 + h, x0:x0 + w])
    rep = hyper_model.last_decompress_report
    assert count == len(tiling.region_tiles(tiling.tile_grid(HH, WW, TILE, 16), region))
    assert rep["tiles_total"] == 12 and rep["tiles_decoded"] == N * count and rep["bytes_total"] == len(blob)
    if count == 1:
        assert rep["tiles_decoded"] < rep["tiles_total"] and rep["bytes_read"] < rep["bytes_total"]


def test_region_refusals(hyper_model, picture, tiled16):
    blob, _ = tiled16
    for region in ((0, 0, 201, 10), (-1, 0, 5, 5), (0, 149, 1, 2), (0, 0, 0, 5)):
        with pytest.raises(ValueError, match="region"):
            hyper_model.decompress(blob, region=region)
    with pytest.raises(ValueError, match="not tiled"):
        hyper_model.decompress(hyper_model.compress(picture[:1, :64, :64]), region=(0, 0, 8, 8))


def test_select_images_on_a_real_batch(hyper_model, dev):
    from shallow_ntc_amd import entropy_coding as ec
    blob = hyper_model.compress(images(3, 64, 64, dev, seed=5))
    full = hyper_model.decompress(blob).cpu().numpy()
    np.testing.assert_array_equal(hyper_model.decompress(ec.select_images(blob, [2, 0])).cpu().numpy(), full[[2, 0]])


@pytest.mark.parametrize("step", [4, [-3, 5]], ids=["one-step", "per-image"])
def test_steps_travel_in_v5_inner_blobs(hyper_model, picture, step):
    from shallow_ntc_amd import entropy_coding as ec
    from shallow_ntc_amd import tiling
    blob = hyper_model.compress(picture, tile=TILE, overlap=16, step=step)
    hd = tiling.parse_v9(blob, 0)
    per_image = step if isinstance(step, list) else [step] * N
    codec = hyper_model._get_codec()
    for b in hd["blobs"]:
        inner = blob[b["at"]:b["at"] + b["bytes"]]
        assert inner[4] == ec.VERSION_STEP
        assert ec.parse_v3(inner, "fp32", codec.latent_shapes)["steps"] == [per_image[i] for i, _, _ in b["tiles"]]
    want_blobs, tiles = decode_tiles(hyper_model, picture, 16, step=step)
    assert [blob[b["at"]:b["at"] + b["bytes"]] for b in hd["blobs"]] == want_blobs
    want, _ = tile_cases.assemble(tiles, N, HH, WW, 3, TILE, 16)
    np.testing.assert_array_equal(hyper_model.decompress(blob).cpu().numpy(), want)


def test_decompress_many_mixes_tiled_and_untiled(hyper_model, picture, tiled16):
    blob, full = tiled16
    plain = hyper_model.compress(picture[:, :96, :80].contiguous())
    alone = hyper_model.decompress(plain).cpu().numpy()
    both = hyper_model.decompress_many([plain, blob, plain])
    np.testing.assert_array_equal(both[0].cpu().numpy(), alone)
    np.testing.assert_array_equal(both[1].cpu().numpy(), full)
    np.testing.assert_array_equal(both[2].cpu().numpy(), alone)


def test_the_decompress_report_does_not_outlive_its_call(hyper_model, picture, tiled16):
    blob, _ = tiled16
    plain = hyper_model.compress(picture[:1, :64, :64].contiguous())
    hyper_model.decompress(blob, region=(5, 7, 30, 40))
    assert hyper_model.last_decompress_report["tiles_decoded"] == N
    hyper_model.decompress(plain)
    assert hyper_model.last_decompress_report is None and hyper_model._get_codec().last_decompress_report is None
    hyper_model.decompress_many([blob, plain, blob])
    rep = hyper_model.last_decompress_report
    assert isinstance(rep, list) and [r["tiles_decoded"] for r in rep] == [12, 12] and rep[0]["bytes_total"] == len(blob)
    hyper_model.decompress_many([plain])
    assert hyper_model.last_decompress_report is None
    hyper_model.decompress(blob)
    with pytest.raises(ValueError, match="region"):
        hyper_model.decompress(blob, region=(0, 0, 201, 10))
    assert hyper_model.last_decompress_report is None


def test_a_flipped_payload_word_is_refused(hyper_model, tiled16):
    from shallow_ntc_amd import _capi as capi
    from shallow_ntc_amd import tiling
    blob, _ = tiled16
    b = tiling.parse_v9(blob, 0)["blobs"][3]
    hd = hyper_model._get_codec()._parse(blob[b["at"]:b["at"] + b["bytes"]])
    assert hd["yw"] > 200
    bad = bytearray(blob)
    bad[b["at"] + hd["pos"] + 2 * hd["zw"] + 2 * (hd["yw"] // 2)] ^= 0x10          # a stream word in the middle of the y payload
    got = None
    with pytest.raises(capi.SntcError, match="bitstream corrupt"):
        got = hyper_model.decompress(bytes(bad))
    assert got is None
    with pytest.raises(capi.SntcError, match="bitstream corrupt"):                 # ... also where the window needs that tile alone
        hyper_model.decompress(bytes(bad), region=(60, 60, 8, 8))


def test_other_entry_points_refuse_tiled_files(hyper_model, fact_model, picture, tiled16):
    from shallow_ntc_amd import _capi as capi
    from shallow_ntc_amd import entropy_coding as ec
    blob, _ = tiled16
    for call in (lambda: hyper_model.transcode(blob, shift=2), lambda: hyper_model.add_residual(blob, picture, 2),
                 lambda: ec.split_residual(blob)):
        with pytest.raises(capi.SntcError, match="format 9|version 9") as e:
            call()
        assert e.value.code == capi.ERR_UNSUPPORTED
    with pytest.raises(ValueError, match="only step may accompany tile, not max_error"):
        hyper_model.compress(picture, tile=TILE, max_error=2)
    with pytest.raises(NotImplementedError, match="tile"):
        fact_model.compress(picture, tile=TILE)
    with pytest.raises(capi.SntcError):
        fact_model.decompress(blob)


def test_bf16x3_tiled_round_trip(dev, picture):
    from shallow_ntc_amd import tiling
    from shallow_ntc_amd.mshyper import configs
    from shallow_ntc_amd.mshyper.models import Model
    from test_hip_itinf_bitstream import _spread_scales
    model = _spread_scales(Model(device=dev, precision="bf16x3", **configs.two_layer_syn(rd_lambda=0.02)))
    x = picture[:1, :150, :130].contiguous()
    blob = model.compress(x, tile=TILE, overlap=16)
    hd = tiling.parse_v9(blob, 1)
    assert hd["arith"] == 1 and blob[5] == 1
    full = model.decompress(blob)
    assert tuple(full.shape) == (1, 150, 130, 3)
    xh = x.cpu().numpy()
    g, plan, _ = tiling.tile_plan(1, 150, 130, TILE, 16)
    sliced = tile_cases.extract(xh, TILE, 16)
    tiles = [None] * len(sliced)
    for b in plan:
        ids = [(i * g["R"] + r) * g["C"] + q for i, r, q in b["tiles"]]
        for k, t in zip(ids, model.decompress(model.compress(np.stack([sliced[k] for k in ids]))).cpu().numpy()):
            tiles[k] = t
    want, _ = tile_cases.assemble(tiles, 1, 150, 130, 3, TILE, 16)
    np.testing.assert_array_equal(full.cpu().numpy(), want)
    np.testing.assert_array_equal(model.decompress(blob, region=(60, 60, 20, 30)).cpu().numpy(), want[:, 60:80, 60:90])
    with pytest.raises(Exception, match="fp32"):
        model.compress(x, tile=TILE, step=2)
