"""Tiled files, the host half (no GPU): the geometry of shallow_ntc_amd.tiling against hand-worked cases, against its own promises
at every position, and against csrc/tile_rules.h compiled into tests/tiles_host.cc (plain, and with AddressSanitizer and UBSan
linked into the program itself, as tests/test_gg_pieces_host.py builds its program); the v9 header; ``select_images``; the
argument refusals of ``compress(tile=...)`` that need no device."""
import os
import shutil
import struct
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import tile_cases

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "tiles_host.cc"
AXES = [(15, 8, 0), (15, 8, 2), (16, 8, 2), (17, 8, 1), (23, 8, 2), (33, 8, 2), (9, 8, 2), (5, 8, 2), (200, 64, 16), (150, 64, 0),
        (129, 64, 16), (40, 12, 3), (4096, 512, 16)]


def tiling():
    from shallow_ntc_amd import tiling as t
    return t


def test_tile_grid_hand_worked_cases():
    t = tiling()
    T = 8
    # L = 2 T - 1: one tile, the whole axis
    assert t.axis_tiles(2 * T - 1, T, 2) == [(0, 15, 0, 15)]
    # L = 2 T: two tiles with cores T, T; extents grow by O on the interior side only
    assert t.axis_tiles(2 * T, T, 2) == [(0, 8, 0, 10), (8, 16, 6, 16)]
    # L = 2 T + 1: two tiles, the last core is T + 1
    assert t.axis_tiles(2 * T + 1, T, 2) == [(0, 8, 0, 10), (8, 17, 6, 17)]
    # L < T: one tile
    assert t.axis_tiles(5, T, 2) == [(0, 5, 0, 5)]
    # three tiles: the middle one grows on both sides
    assert t.axis_tiles(3 * T + 3, T, 1) == [(0, 8, 0, 9), (8, 16, 7, 17), (16, 27, 15, 27)]
    g = t.tile_grid(200, 150, 64, 0)
    assert (g["R"], g["C"]) == (3, 2)
    assert [r[2:] for r in g["rows"]] == [(0, 64), (64, 128), (128, 200)] and [c[2:] for c in g["cols"]] == [(0, 64), (64, 150)]
    g = t.tile_grid(200, 150, 64, 16)
    assert [r[2:] for r in g["rows"]] == [(0, 80), (48, 144), (112, 200)] and [c[2:] for c in g["cols"]] == [(0, 80), (48, 150)]
    # the band of the hand-worked rule: T = 8, O = 2, boundary 8, band [6, 10): weights 1 3 5 7 for the right tile, over 8
    assert [t.axis_cover(16, 8, 2, p) for p in (5, 6, 7, 8, 9, 10)] == [
        ([(0, 1)], 1), ([(0, 7), (1, 1)], 8), ([(0, 5), (1, 3)], 8), ([(0, 3), (1, 5)], 8), ([(0, 1), (1, 7)], 8), ([(1, 1)], 1)]
    for bad in ((16, 6, 0), (16, 8, 3), (16, 8, -1), (0, 8, 0), (16, 2, 0), (16, True, 0), (16, 8.0, 0)):
        with pytest.raises(ValueError):
            t.axis_tiles(*bad)


@pytest.mark.parametrize("L,T,O", AXES)
def test_every_position_is_covered_and_the_weights_sum_to_the_denominator(L, T, O):
    t = tiling()
    tiles = t.axis_tiles(L, T, O)
    assert len(tiles) == max(1, L // T)
    assert tiles[0][0] == 0 and tiles[-1][1] == L and all(a[1] == b[0] for a, b in zip(tiles, tiles[1:]))       # cores partition
    assert all(e1 - e0 >= min(L, T) for _, _, e0, e1 in tiles)
    w, den = tile_cases.axis_weights(L, T, O)              # the independent restatement
    for p in range(L):
        cover, d = t.axis_cover(L, T, O, p)
        inside = [r for r, (_, _, e0, e1) in enumerate(tiles) if e0 <= p < e1]
        assert [r for r, _ in cover] == inside and len(inside) in (1, 2)
        assert all(wt >= 1 for _, wt in cover) and sum(wt for _, wt in cover) == d == den[p]
        assert [(r, int(w[r, p])) for r in inside] == cover
    assert [e for _, _, *e in tiles] == [list(e) for e in tile_cases.extents(L, T, O)]


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if cxx and shutil.which(cxx):
            return cxx
    pytest.fail("no host C++ compiler (g++ / c++ / clang++) on PATH")


SANITIZE = ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


@pytest.mark.parametrize("flags", [("-O2",), SANITIZE], ids=["plain", "asan-ubsan"])
def test_the_header_the_kernels_compile_prints_the_same_tables(flags, tmp_path):
    t = tiling()
    exe = tmp_path / "tiles_host"
    cxx = _compiler()
    if flags is SANITIZE and "clang" not in cxx:
        flags = flags + ("-static-libasan", "-static-libubsan")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", *flags, str(SRC), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)] + [str(v) for axis in AXES for v in axis] + ["16", "6", "0"], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert " 0 mismatches" in r.stdout and "invalid 16 6 0" in r.stdout
    want = []
    for L, T, O in AXES:
        tiles = t.axis_tiles(L, T, O)
        want.append(f"axis {L} {T} {O} {len(tiles)}")
        want += [f"tile {k} {e0} {e1}" for k, (_, _, e0, e1) in enumerate(tiles)]
        for p in range(L):
            cover, den = t.axis_cover(L, T, O, p)
            two = len(cover) - 1
            want.append(f"pos {p} {cover[0][0]} {two} {cover[0][1]} {cover[1][1] if two else 0} {den}")
    got = [ln for ln in r.stdout.splitlines() if ln.split()[0] in ("axis", "tile", "pos")]
    assert got == want
    text = (ROOT / "shallow-ntc_amd" / "csrc" / "tiles.hip").read_text()
    assert '#include "tile_rules.h"' in text and "tile_cover(" in text and "tile_blend(" in text
    make = (ROOT / "shallow-ntc_amd" / "csrc" / "Makefile").read_text()
    assert "tile_rules.h" in make and "tiles.hip" in make


# -- wire format 9 -------------------------------------------------------------------------------------------------------
DIMS = (8, 4, 1, 1, 4, 4)                        # (C, Cz, hz, wz, h, w): made up; pack_v3 does not judge them


def inner_blob(ec, rng, count, th, tw, arith=0, steps=None):
    zl, yl = rng.integers(1, 9, count), rng.integers(1, 30, count)
    words = rng.integers(0, 1 << 16, int(zl.sum() + yl.sum()), dtype=np.uint16)
    return ec.pack_v3(arith, count, th, tw, DIMS, 1, 1, 8, 8, zl, yl, steps) + words.astype("<u2").tobytes()


def tiled_file(n=2, H=200, W=150, T=64, O=16, arith=0, seed=0):
    from shallow_ntc_amd import entropy_coding as ec
    t = tiling()
    rng = np.random.default_rng(seed)
    _, plan, _ = t.tile_plan(n, H, W, T, O)
    inner = [inner_blob(ec, rng, len(b["tiles"]), b["th"], b["tw"], arith) for b in plan]
    return t.pack_v9(arith, n, H, W, T, O, inner), plan, inner


def test_v9_pack_parse_round_trip_and_tile_index():
    t = tiling()
    blob, plan, inner = tiled_file()
    assert t.is_tiled(blob) and not t.is_tiled(inner[0]) and blob[4] == t.VERSION_TILED == 9
    hd = t.parse_v9(blob, 0)
    assert (hd["n"], hd["H"], hd["W"], hd["tile"], hd["overlap"], hd["arith"]) == (2, 200, 150, 64, 16, 0)
    assert [blob[b["at"]:b["at"] + b["bytes"]] for b in hd["blobs"]] == inner
    # 3 x 2 tiles per image; shapes in order of first appearance: (80, 80) (80, 102) (96, 80) (96, 102) (88, 80) (88, 102)
    assert [(b["th"], b["tw"], len(b["tiles"])) for b in plan] == [(80, 80, 2), (80, 102, 2), (96, 80, 2), (96, 102, 2), (88, 80, 2), (88, 102, 2)]
    idx = t.tile_index(blob)
    assert (idx["R"], idx["C"], len(idx["tiles"])) == (3, 2, 12)
    assert idx["tiles"][0] == dict(image=0, row=0, col=0, y0=0, y1=80, x0=0, x1=80, blob=0, index=0)
    assert idx["tiles"][9] == dict(image=1, row=1, col=1, y0=48, y1=144, x0=48, x1=150, blob=3, index=1)
    # overlap 0, one shape class cut every TILE_BATCH tiles: 2 x 20 x 16 tiles of 64 x 64 = 640 -> 256 + 256 + 128
    _, plan, where = t.tile_plan(2, 64 * 20, 64 * 16, 64, 0)
    assert [(b["th"], b["tw"], len(b["tiles"])) for b in plan] == [(64, 64, 256), (64, 64, 256), (64, 64, 128)]
    assert where[1, 19, 15].tolist() == [2, 127] and where[0, 16, 0].tolist() == [1, 0] and plan[1]["tiles"][0] == (0, 16, 0)


def test_v9_refusals():
    from shallow_ntc_amd import _capi as capi
    from shallow_ntc_amd import entropy_coding as ec
    t = tiling()
    blob, plan, inner = tiled_file()
    head = 4 + struct.calcsize(t.HEAD_V9)
    esize = struct.calcsize(t.ENTRY_V9)

    def refused(b, code, text):
        with pytest.raises(capi.SntcError, match=text) as e:
            t.parse_v9(bytes(b), 0)
        assert e.value.code == code

    refused(blob[:-1], capi.ERR_BAD_SHAPE, "truncated")
    refused(blob[:head + 3], capi.ERR_BAD_SHAPE, "truncated")
    refused(blob[:10], capi.ERR_BAD_SHAPE, "truncated")
    refused(blob + b"\0", capi.ERR_BAD_SHAPE, "followed by bytes")
    refused(b"XNTC" + blob[4:], capi.ERR_BAD_SHAPE, "not an SNTC")
    # wrong entry table: th of entry 1, count of entry 0
    b = bytearray(blob)
    struct.pack_into("<H", b, head + esize, 81)
    refused(b, capi.ERR_BAD_SHAPE, "entry 1")
    b = bytearray(blob)
    struct.pack_into("<I", b, head + 4, 3)
    refused(b, capi.ERR_BAD_SHAPE, "entry 0")
    # nblobs off by one, either way
    for d in (-1, 1):
        b = bytearray(blob)
        struct.pack_into("<H", b, head - 2, len(plan) + d)
        refused(b, capi.ERR_BAD_SHAPE, "inner blobs")
    # geometry outside the rule, implausible sizes
    for off, fmt, v, text in ((head - 6, "<H", 62, "outside the rule"), (head - 4, "<H", 17, "outside the rule"), (6, "<H", 0, "implausible")):
        b = bytearray(blob)
        struct.pack_into(fmt, b, off, v)
        refused(b, capi.ERR_BAD_SHAPE, text)
    # arithmetic: the reader's, and an inner blob of another one
    with pytest.raises(capi.SntcError, match="arithmetic") as e:
        t.parse_v9(blob, 1)
    assert e.value.code == capi.ERR_UNSUPPORTED
    rng = np.random.default_rng(1)
    other = list(inner)
    other[2] = inner_blob(ec, rng, 2, plan[2]["th"], plan[2]["tw"], arith=1)
    refused(t.pack_v9(0, 2, 200, 150, 64, 16, other), capi.ERR_BAD_SHAPE, "different arithmetics")
    # an inner blob of another count / size / version
    other = list(inner)
    other[0] = inner_blob(ec, rng, 3, 80, 80)
    refused(t.pack_v9(0, 2, 200, 150, 64, 16, other), capi.ERR_BAD_SHAPE, "inner blob 0 holds 3 images")
    other[0] = inner[0][:4] + bytes([7]) + inner[0][5:]
    refused(t.pack_v9(0, 2, 200, 150, 64, 16, other), capi.ERR_UNSUPPORTED, "version 7 inner blob")
    refused(inner[0], capi.ERR_UNSUPPORTED, "version 3")
    with pytest.raises(ValueError):
        t.pack_v9(0, 2, 200, 150, 64, 16, inner[:-1])
    # the other readers name the format
    with pytest.raises(capi.SntcError, match="version 9") as e:
        ec.split_residual(blob)
    assert e.value.code == capi.ERR_UNSUPPORTED


def test_v9_hostile_headers_are_refused_before_anything_is_built(monkeypatch):
    """A 22-byte header may name 10^12 tiles.  The reader counts tiles and inner blobs by arithmetic, holds the file to the
    writer's tile >= 64, and builds the plan only once the blob is long enough to hold it: ``tile_plan`` is never reached."""
    from shallow_ntc_amd import _capi as capi
    t = tiling()

    def never(*a, **k):
        raise AssertionError("tile_plan was built from an unchecked header")

    head = lambda n, H, W, tile, overlap, nblobs: b"SNTC" + struct.pack(t.HEAD_V9, 9, n, H, W, tile, overlap, nblobs)
    # the counts by arithmetic are the plan's
    for case in ((2, 200, 150, 64, 16), (2, 1280, 1024, 64, 0), (3, 129, 700, 64, 8), (1, 63, 64, 64, 16), (5, 4096, 4096, 512, 16)):
        _, plan, _ = t.tile_plan(*case)
        assert t.plan_counts(*case) == (sum(len(b["tiles"]) for b in plan), len(plan)), case
    assert t.plan_counts(4096, 65536, 65536, 64, 0) == (4096 * 1024 * 1024, 4096 * 1024 * 1024 // 256)
    monkeypatch.setattr(t, "tile_plan", never)
    for hostile, text in ((head(4096, 65536, 65536, 4, 0, 1), "at least 64"), (head(4096, 65536, 65536, 64, 0, 1), "inner blobs"),
                          (head(4096, 65536, 65536, 64, 16, 65535), "inner blobs"), (head(1, 65536, 65536, 60, 0, 1), "at least 64"),
                          # the right count of inner blobs for 16 x 1024 x 1024 tiles, and nothing behind the header
                          (head(16, 65536, 65536, 64, 0, 65536 - 1), "inner blobs"),
                          (head(1, 8192, 8192, 64, 0, 64), "truncated"),
                          (head(1, 8192, 8192, 64, 0, 64) + bytes(64 * 12), "truncated"),
                          (head(1, 8192, 8192, 64, 0, 64) + bytes(64 * (12 + 34) + 8 * 128 * 128 - 1), "truncated")):
        with pytest.raises(capi.SntcError, match=text) as e:
            t.parse_v9(hostile, 0)
        assert e.value.code == capi.ERR_BAD_SHAPE
        with pytest.raises(capi.SntcError, match=text):
            t.tile_index(hostile)


def test_the_format_constants_are_entropy_codings():
    """tiling.py is a leaf module (entropy_coding imports it), so it spells these out again."""
    from shallow_ntc_amd import entropy_coding as ec
    t = tiling()
    assert (t.MAGIC, t.HEAD_V3, t.MAX_IMAGES, t.MAX_SIDE) == (ec.MAGIC, ec.HEAD_V3, ec.Codec.MAX_IMAGES, ec.Codec.MAX_SIDE)
    assert (ec.VERSION, ec.VERSION_STEP, ec.VERSION_TILED, ec.tiling.TILE_MIN_FILE) == (3, 5, t.VERSION_TILED, 64)
    assert 4 + struct.calcsize(t.HEAD_V3) == 34 and t.TILE_BYTES_MIN == 2 * 4


# -- select_images -------------------------------------------------------------------------------------------------------
BIG = (320, 192, 8, 8, 32, 32)                   # 327 680 y elements = 2 segments, 12 288 z elements = 1 segment


def batch_blob(ec, n, steps=None, seed=0):
    rng = np.random.default_rng(seed)
    ez, ey = BIG[1] * BIG[2] * BIG[3], BIG[0] * BIG[4] * BIG[5]
    sz, sy = ec._segments(ez), ec._segments(ey)
    assert (sz, sy) == (1, 2)
    lz, ly = ec._lanes(-(-ez // sz)), ec._lanes(-(-ey // sy))
    zl, yl = rng.integers(0, 7, n * sz), rng.integers(0, 40, n * sy)
    zw, yw = (rng.integers(0, 1 << 16, int(l.sum()), dtype=np.uint16) for l in (zl, yl))
    blob = ec.pack_v3(0, n, 512, 512, BIG, sz, sy, lz, ly, zl, yl, steps) + zw.astype("<u2").tobytes() + yw.astype("<u2").tobytes()
    return blob, zl.reshape(n, sz), yl.reshape(n, sy), zw, yw


@pytest.mark.parametrize("steps", [None, [3, -2, 0, 7, 1]], ids=["v3", "v5"])
@pytest.mark.parametrize("idx", [[2, 0], [4], [1, 1, 3, 1], [4, 3, 2, 1, 0], [0, 1, 2, 3]])
def test_select_images_keeps_lengths_steps_and_word_slices(steps, idx):
    from shallow_ntc_amd import entropy_coding as ec
    n = 5
    blob, zl, yl, zw, yw = batch_blob(ec, n, steps)
    shapes = lambda H, W: BIG
    src = ec.parse_v3(blob, "fp32", shapes)
    assert src["steps"] == steps
    out = ec.select_images(blob, idx)
    hd = ec.parse_v3(out, "fp32", shapes)
    assert hd["n"] == len(idx) and (hd["H"], hd["W"], hd["sz"], hd["sy"], hd["lz"], hd["ly"]) == (512, 512, src["sz"], src["sy"], src["lz"], src["ly"])
    assert hd["zl"].tolist() == zl[idx].reshape(-1).tolist() and hd["yl"].tolist() == yl[idx].reshape(-1).tolist()
    assert hd["steps"] == (None if steps is None else [steps[i] for i in idx])
    zo, yo = np.concatenate([[0], np.cumsum(zl.sum(axis=1))]), np.concatenate([[0], np.cumsum(yl.sum(axis=1))])
    words = np.frombuffer(out, "<u2", offset=hd["pos"])
    want = np.concatenate([zw[zo[i]:zo[i + 1]] for i in idx] + [yw[yo[i]:yo[i + 1]] for i in idx])
    assert words.tolist() == want.tolist()
    assert out[:4] == blob[:4] and out[4:6] == blob[4:6] and out[8:4 + struct.calcsize(ec.HEAD_V3)] == blob[8:4 + struct.calcsize(ec.HEAD_V3)]


def test_select_images_identity_and_refusals():
    from shallow_ntc_amd import _capi as capi
    from shallow_ntc_amd import entropy_coding as ec
    blob, *_ = batch_blob(ec, 3, [1, 2, 3])
    assert ec.select_images(blob, [0, 1, 2]) is blob or ec.select_images(blob, [0, 1, 2]) == blob
    assert ec.select_images(ec.select_images(blob, [2, 0, 1]), [1, 2, 0]) == blob
    for idx in ([], [3], [-1], [0, 5]):
        with pytest.raises(ValueError):
            ec.select_images(blob, idx)
    for ver in (7, 8, 4, 9):
        with pytest.raises(capi.SntcError, match=f"version {ver}") as e:
            ec.select_images(blob[:4] + bytes([ver]) + blob[5:], [0])
        assert e.value.code == capi.ERR_UNSUPPORTED
    for cut in (blob[:-2], blob + b"\0\0", blob[:20], blob[:5]):
        with pytest.raises(capi.SntcError, match="truncated"):
            ec.select_images(cut, [0])
    tiled, _, _ = tiled_file()
    with pytest.raises(capi.SntcError, match="version 9"):
        ec.select_images(tiled, [0])


# -- compress(tile=...): the refusals that come before any device work -----------------------------------------------------------
def test_compress_tile_argument_refusals():
    from shallow_ntc_amd import entropy_coding as ec
    from shallow_ntc_amd.factorized.models import Model as FactorizedModel
    from shallow_ntc_amd.mshyper.models import Model
    t = tiling()
    assert t.check_tiling(64, 16, 16) == (64, 16) and t.check_tiling(512, 0, 16) == (512, 0) and t.check_tiling(np.int64(128), 32, 16) == (128, 32)
    for tile, overlap in ((48, 0), (72, 0), (64, 17), (64, -1), (63, 0), (64.0, 0), (True, 0), (64, None), (65536, 0), (8192, 1025)):
        with pytest.raises(ValueError):
            t.check_tiling(tile, overlap, 16)
    stub = SimpleNamespace(factorized=False, downsample_factor=16)         # refused before the model is touched
    x = np.zeros((1, 128, 128, 3), np.float32)
    for name, value in (("itinf", dict(steps=2)), ("target_bpp", 0.5), ("target_psnr", 30.0), ("max_error", 2), ("rdoq", True),
                        ("step_offsets", np.zeros((1, 8, 8), np.int8))):
        with pytest.raises(ValueError, match=f"only step may accompany tile, not {name}"):
            Model.compress(stub, x, tile=64, **{name: value})
    for tile, overlap in ((48, 0), (72, 16), (64, 17)):
        with pytest.raises(ValueError, match="tile|overlap"):
            Model.compress(stub, x, tile=tile, overlap=overlap)
    with pytest.raises(NotImplementedError, match="tile"):
        FactorizedModel.compress(SimpleNamespace(factorized=True), x, tile=64)
    codec = object.__new__(ec.Codec)
    codec.m = SimpleNamespace(downsample_factor=16)
    for kw in (dict(target_bpp=1.0), dict(target_psnr=30.0), dict(step_offsets=np.zeros((1, 8, 8), np.int8))):
        with pytest.raises(ValueError, match="only step may accompany tile"):
            ec.Codec.compress(codec, x, tile=64, **kw)
    with pytest.raises(ValueError, match="tile 88"):
        ec.Codec.compress(codec, x, tile=88, overlap=0)
    # the Codec entry refuses before the upload too: this stub has no ``_as_device_images`` to reach
    for kw, text in ((dict(step=99), "ladder index"), (dict(step=[1, 2]), "2 steps for 1 images"), (dict(step=1.5), "step")):
        with pytest.raises(ValueError, match=text):
            ec.Codec.compress(codec, x, tile=64, overlap=16, **kw)
    with pytest.raises(ValueError, match="shape"):
        ec.Codec.compress(codec, np.zeros((128, 128), np.float32), tile=64)
    codec.m._precision = "bf16x3"
    with pytest.raises(Exception, match="fp32"):
        ec.Codec.compress(codec, x, tile=64, overlap=16, step=2)
    with pytest.raises(ValueError, match="region"):
        t.region_tiles(t.tile_grid(200, 150, 64, 16), (0, 0, 201, 10))
    with pytest.raises(ValueError, match="region"):
        t.region_tiles(t.tile_grid(200, 150, 64, 16), (10, 140, 5, 11))
    g = t.tile_grid(200, 150, 64, 16)
    assert t.region_tiles(g, (0, 0, 48, 48)) == [(0, 0)] and t.region_tiles(g, (0, 0, 49, 49)) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert t.region_tiles(g, (199, 149, 1, 1)) == [(2, 1)] and len(t.region_tiles(g, (0, 0, 200, 150))) == 6
