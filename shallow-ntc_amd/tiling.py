"""Tiled files (wire format 9, DESIGN.md 4.7 "tiled files"): the host half.  No function here touches a device.

A picture is cut into overlapping tiles, the tiles are coded as the images of ordinary v3 / v5 batches -- an image of a batch
encodes and decodes bit-identically whatever else is in the batch, and its rANS streams have explicit lengths, so a tile can be
cut out of its batch (``select_images``) and decoded alone, exactly -- and decoded tiles are blended across their seams.  The
reference never writes a file (mshyper/models.py:246-251) and has no tiles.

Geometry, per axis, for a length L, a tile size T and an overlap O (csrc/tile_rules.h is the definition the kernels compile; this
module restates it and tests/test_tiling_host.py compares the two):
  R = max(1, L // T); the core of tile r is [r T, (r + 1) T) for r < R - 1, the last core runs to L (its length lies in [T, 2 T));
  the extent of tile r is its core grown by O on each interior side, clipped to [0, L); with T >= 4, T % 4 == 0 and
  0 <= O <= min(T / 4, 1024) the extents of r and r + 1 meet exactly in the band [(r + 1) T - O, (r + 1) T + O), bands are disjoint,
  and every position outside a band lies in exactly one extent.  At band offset j tile r + 1 weighs 2 j + 1 and tile r weighs
  4 O - (2 j + 1) over the denominator 4 O; elsewhere the one tile weighs 1 over 1.  In 2-D the weight is the product of the axis
  weights, D = Dy Dx, and an output value is (sum_t w_t v_t + D // 2) // D in integers.

Wire format 9 (little endian):
  b"SNTC" | u16 (9 | arith << 8) | u16 n | u32 H | u32 W | u16 tile | u16 overlap | u16 nblobs |
  nblobs x (u16 th, u16 tw, u32 count, u32 bytes) | the inner blobs
Tiles are ordered (image, row, column), grouped by shape (th, tw) in order of first appearance, and each group is cut into
consecutive inner blobs of at most TILE_BATCH tiles; an inner blob is an ordinary v3 / v5 file of ``count`` images of th x tw.
``parse_v9`` recomputes the whole entry table from (n, H, W, tile, overlap) and refuses any mismatch: nothing later trusts the
header."""
from __future__ import annotations

import struct
from collections import Counter

import numpy as np

from . import _capi as capi

MAGIC = b"SNTC"
VERSION_TILED = 9
TILE_BATCH = 256                          # tiles of one inner blob at the most
TILE_MIN, OVERLAP_MAX = 4, 1024           # kTileMin, kTileMaxOverlap of csrc/tile_rules.h
TILE_MIN_FILE = 64                        # the smallest tile a FILE carries: the writer's bound, and the reader's
TILE_BYTES_MIN = 8                        # what every tile costs its inner blob at the very least: one u32 length field per latent
HEAD_V9 = "<HHIIHHH"                      # version | n | H | W | tile | overlap | nblobs
ENTRY_V9 = "<HHII"                        # th | tw | count | bytes
HEAD_V3 = "<HHIIHHHHHHHHBB"               # entropy_coding.HEAD_V3: what ``select_images`` reads of an inner blob
MAX_IMAGES, MAX_SIDE = 4096, 1 << 16      # entropy_coding.Codec's limits


def check_tile(L, tile, overlap):
    """The C-level validity of one axis (``tile_valid``): ValueError otherwise."""
    for name, v in (("length", L), ("tile", tile), ("overlap", overlap)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"tiles: {name} must be an int, not {v!r}")
    if L < 1 or tile < TILE_MIN or tile % 4 or not 0 <= overlap <= min(tile // 4, OVERLAP_MAX):
        raise ValueError(f"tiles: length {L} >= 1, tile {tile} >= {TILE_MIN} and a multiple of 4, "
                         f"0 <= overlap {overlap} <= min(tile / 4, {OVERLAP_MAX})")


def check_tiling(tile, overlap, factor):
    """``tile`` / ``overlap`` of ``compress`` -> (T, O) as ints; ValueError unless T is a multiple of ``factor`` (the model's
    downsample factor, 64 for the hyperprior models) with TILE_MIN_FILE <= T <= 65532 and 0 <= O <= min(T / 4, OVERLAP_MAX).
    A tile is padded like any image, up to the next multiple of ``factor``: a CORE of T pixels wastes nothing, but what is coded
    is the EXTENT, T + O or T + 2 O pixels, which is padded to T + factor whenever 0 < 2 O < factor -- at T = 256, O = 16,
    factor 64 every tile is coded as 320 x 320, 1.56 x the core's pixels (DESIGN.md 4.7 has the measured price).  O = factor / 2
    makes interior extents pad-free; O = 0 costs only the per-tile overheads."""
    for name, v in (("tile", tile), ("overlap", overlap)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"compress: {name} must be an int, not {v!r}")
    T, O, f = int(tile), int(overlap), int(factor)
    if T < TILE_MIN_FILE or T % f or T % 4 or T > 0xfffc:
        raise ValueError(f"compress: tile {T} must be a multiple of the model's downsample factor {f} (and of 4), at least "
                         f"{TILE_MIN_FILE} and at most 65532")
    if not 0 <= O <= min(T // 4, OVERLAP_MAX):
        raise ValueError(f"compress: overlap {O} outside [0, min(tile / 4, {OVERLAP_MAX})] = [0, {min(T // 4, OVERLAP_MAX)}]")
    return T, O


def refuse_with_tile(**given):
    """``compress(x, tile=...)`` takes ``step`` alone: ValueError naming every other option in ``given`` that is not None."""
    extra = [k for k, v in given.items() if v is not None and v is not False]
    if extra:
        raise ValueError(f"compress: only step may accompany tile, not {', '.join(extra)}")


def axis_tiles(L, tile, overlap):
    """One axis -> per tile (core_begin, core_end, extent_begin, extent_end)."""
    check_tile(L, tile, overlap)
    L, T, O = int(L), int(tile), int(overlap)
    R = max(1, L // T)
    out = []
    for r in range(R):
        c0, c1 = r * T, (L if r == R - 1 else (r + 1) * T)
        out.append((c0, c1, 0 if r == 0 else c0 - O, L if r == R - 1 else c1 + O))
    return out


def axis_cover(L, tile, overlap, p):
    """The tiles whose extents hold position p of an axis -> ([(tile, weight), ...] of one or two entries, denominator)."""
    T, O = int(tile), int(overlap)
    R = max(1, int(L) // T)
    k, j = divmod(int(p) + O, T)
    if 1 <= k <= R - 1 and j < 2 * O:
        return [(k - 1, 4 * O - (2 * j + 1)), (k, 2 * j + 1)], 4 * O
    return [(min(int(p) // T, R - 1), 1)], 1


def tile_grid(H, W, tile, overlap):
    """-> dict(R, C, rows, cols): ``rows`` / ``cols`` = ``axis_tiles`` of the two axes (core and extent of every tile row /
    column); tile (r, c) of an image covers rows[r][2:4] x cols[c][2:4]."""
    rows, cols = axis_tiles(H, tile, overlap), axis_tiles(W, tile, overlap)
    return dict(R=len(rows), C=len(cols), rows=rows, cols=cols, H=int(H), W=int(W), tile=int(tile), overlap=int(overlap))


def tile_plan(n, H, W, tile, overlap):
    """How the n R C tiles of a file are laid into inner blobs -> (grid, blobs, where): ``blobs`` = list of dict(th, tw, tiles =
    [(image, row, col), ...]) in file order; ``where`` int64 [n, R, C, 2] = (inner blob, index within it) of every tile.  Tiles
    in (image, row, col) order, grouped by shape in order of first appearance, each group cut every TILE_BATCH tiles."""
    g = tile_grid(H, W, tile, overlap)
    groups = {}
    for i in range(int(n)):
        for r, (_, _, y0, y1) in enumerate(g["rows"]):
            for c, (_, _, x0, x1) in enumerate(g["cols"]):
                groups.setdefault((y1 - y0, x1 - x0), []).append((i, r, c))
    blobs = []
    where = np.zeros((int(n), g["R"], g["C"], 2), np.int64)
    for (th, tw), tiles in groups.items():
        for lo in range(0, len(tiles), TILE_BATCH):
            part = tiles[lo:lo + TILE_BATCH]
            for k, (i, r, c) in enumerate(part):
                where[i, r, c] = (len(blobs), k)
            blobs.append(dict(th=th, tw=tw, tiles=part))
    return g, blobs, where


def plan_counts(n, H, W, tile, overlap):
    """(tiles, inner blobs) of ``tile_plan(n, H, W, tile, overlap)`` WITHOUT building it: per axis the extents' lengths are
    counted (R + C entries), a shape class (th, tw) holds n x count(th) x count(tw) tiles and is cut every TILE_BATCH.  What a
    reader computes before it trusts a header with anything larger."""
    hs = Counter(e1 - e0 for _, _, e0, e1 in axis_tiles(H, tile, overlap))
    ws = Counter(e1 - e0 for _, _, e0, e1 in axis_tiles(W, tile, overlap))
    tiles = int(n) * sum(hs.values()) * sum(ws.values())
    return tiles, sum(-(-int(n) * a * b // TILE_BATCH) for a in hs.values() for b in ws.values())


def is_tiled(blob) -> bool:
    """Whether ``blob`` announces wire format 9 (its version byte; nothing else is checked)."""
    return len(blob) > 4 and bytes(blob[:4]) == MAGIC and blob[4] == VERSION_TILED


def pack_v9(arith, n, H, W, tile, overlap, inner) -> bytes:
    """The file of the inner blobs ``inner`` (in ``tile_plan`` order).  ValueError where they are not the plan's count."""
    _, blobs, _ = tile_plan(n, H, W, tile, overlap)
    if len(inner) != len(blobs) or len(blobs) > 0xffff:
        raise ValueError(f"pack_v9: {len(inner)} inner blobs for a plan of {len(blobs)}")
    if max(b["th"] for b in blobs) > 0xffff or max(b["tw"] for b in blobs) > 0xffff:
        raise ValueError("pack_v9: a tile extent beyond 65535")
    head = MAGIC + struct.pack(HEAD_V9, VERSION_TILED | (int(arith) << 8), n, H, W, tile, overlap, len(blobs))
    table = b"".join(struct.pack(ENTRY_V9, b["th"], b["tw"], len(b["tiles"]), len(data)) for b, data in zip(blobs, inner))
    return head + table + b"".join(bytes(d) for d in inner)


def parse_v9(blob, arith=None):
    """Header and entry table of a v9 blob, every entry recomputed from (n, H, W, tile, overlap) -> dict(arith, n, H, W, tile,
    overlap, grid, blobs (``tile_plan``'s, each with at = its offset and bytes = its size in the file), where, head_bytes).
    Nothing is built or allocated from the header before the blob has shown that it can hold it (``plan_counts``): the work is
    linear in the length of the blob, whatever its 22 header bytes say.
    Refused (SntcError): another version or, with ``arith`` given, another arithmetic (ERR_UNSUPPORTED); an implausible size, a
    tile / overlap outside the rule or a tile below TILE_MIN_FILE, an inner-blob count that is not the geometry's, a blob shorter
    than its entry table + a header per inner blob + TILE_BYTES_MIN bytes per tile, an entry table that is not the plan's, an inner blob that is not a v3 / v5 file of the
    entry's count, size and the header's arithmetic, truncation, trailing bytes (ERR_BAD_SHAPE)."""
    bad = lambda what: capi.SntcError(capi.ERR_BAD_SHAPE, f"bitstream header: tiled file {what}")
    if bytes(blob[:4]) != MAGIC:
        raise capi.SntcError(capi.ERR_BAD_SHAPE, "not an SNTC bitstream")
    pos = 4 + struct.calcsize(HEAD_V9)
    if len(blob) < pos:
        raise capi.SntcError(capi.ERR_BAD_SHAPE, "bitstream truncated")
    word, n, H, W, tile, overlap, nblobs = struct.unpack_from(HEAD_V9, blob, 4)
    tag, ver = word >> 8, word & 0xff
    if ver != VERSION_TILED:
        raise capi.SntcError(capi.ERR_UNSUPPORTED, f"bitstream version {ver}: a tiled file is version {VERSION_TILED}")
    if arith is not None and tag != arith:
        raise capi.SntcError(capi.ERR_UNSUPPORTED, f"tiled bitstream (wire format {VERSION_TILED}) was written in arithmetic {tag}, this model "
                             f"computes in arithmetic {arith}: mu / sigma would not be reproduced bit for bit")
    if not (1 <= n <= MAX_IMAGES and 1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise capi.SntcError(capi.ERR_BAD_SHAPE, f"bitstream header: implausible batch / image size n={n} H={H} W={W}")
    try:
        check_tile(H, tile, overlap)
        check_tile(W, tile, overlap)
    except ValueError as e:
        raise bad(f"names a tile size / overlap outside the rule ({e})") from None
    if tile < TILE_MIN_FILE:
        raise bad(f"names tile size {tile}; a file's tiles are at least {TILE_MIN_FILE}")
    # Nothing is built from the header before the blob itself has shown that it can hold it: the tile and inner-blob counts come
    # from arithmetic on at most H / tile + W / tile <= 2048 axis entries, the blob must announce that many inner blobs, and it
    # must be long enough for the entry table, a header per inner blob and TILE_BYTES_MIN bytes per tile.  The plan built below
    # is then linear in the length of the blob.
    ntiles, want = plan_counts(n, H, W, tile, overlap)
    if nblobs != want:
        raise bad(f"announces {nblobs} inner blobs, its geometry gives {want}")
    esize = struct.calcsize(ENTRY_V9)
    small = 4 + struct.calcsize(HEAD_V3)
    if len(blob) < pos + nblobs * (esize + small) + ntiles * TILE_BYTES_MIN:
        raise capi.SntcError(capi.ERR_BAD_SHAPE, "bitstream truncated")
    grid, blobs, where = tile_plan(n, H, W, tile, overlap)
    assert len(blobs) == nblobs
    at = pos + nblobs * esize
    for k, b in enumerate(blobs):
        th, tw, count, size = struct.unpack_from(ENTRY_V9, blob, pos + k * esize)
        if (th, tw, count) != (b["th"], b["tw"], len(b["tiles"])):
            raise bad(f"entry {k} = {(th, tw, count)} (th, tw, count), its geometry gives {(b['th'], b['tw'], len(b['tiles']))}")
        if size < small:
            raise bad(f"entry {k} announces {size} bytes, less than a header")
        if len(blob) < at + size:
            raise capi.SntcError(capi.ERR_BAD_SHAPE, "bitstream truncated")
        if bytes(blob[at:at + 4]) != MAGIC:
            raise bad(f"holds no SNTC bitstream as inner blob {k}")
        iword, inn, iH, iW = struct.unpack_from("<HHII", blob, at + 4)
        if iword & 0xff not in (3, 5):
            raise capi.SntcError(capi.ERR_UNSUPPORTED, f"bitstream header: tiled file over a version {iword & 0xff} inner blob; an inner "
                                 "blob is version 3 or 5")
        if iword >> 8 != tag:
            raise bad(f"and its inner blob {k} name different arithmetics")
        if (inn, iH, iW) != (count, th, tw):
            raise bad(f"inner blob {k} holds {inn} images of {iH} x {iW}, its entry says {count} of {th} x {tw}")
        b.update(at=at, bytes=size)
        at += size
    if len(blob) != at:
        raise bad("is followed by bytes it does not announce")
    return dict(arith=tag, n=n, H=H, W=W, tile=tile, overlap=overlap, grid=grid, blobs=blobs, where=where,
                head_bytes=pos + nblobs * esize)


def tile_index(blob):
    """A v9 blob -> dict(n, H, W, tile, overlap, R, C, rows, cols, tiles): ``tiles`` = per tile, in (image, row, col) order,
    dict(image, row, col, y0, y1, x0, x1 (its extent), blob (its inner blob), index (within it)); host only."""
    hd = parse_v9(blob)
    g = hd["grid"]
    tiles = []
    for i in range(hd["n"]):
        for r, (_, _, y0, y1) in enumerate(g["rows"]):
            for c, (_, _, x0, x1) in enumerate(g["cols"]):
                k, j = hd["where"][i, r, c]
                tiles.append(dict(image=i, row=r, col=c, y0=y0, y1=y1, x0=x0, x1=x1, blob=int(k), index=int(j)))
    return dict(n=hd["n"], H=hd["H"], W=hd["W"], tile=hd["tile"], overlap=hd["overlap"], R=g["R"], C=g["C"], rows=g["rows"],
                cols=g["cols"], tiles=tiles)


def region_tiles(grid, region):
    """(y0, x0, h, w) -> the (row, col) of every tile whose extent meets the window; ValueError on a window that is empty or
    leaves the picture."""
    try:
        y0, x0, h, w = (int(v) for v in region)
    except (TypeError, ValueError):
        raise ValueError(f"region must be (y0, x0, h, w), not {region!r}") from None
    if y0 < 0 or x0 < 0 or h < 1 or w < 1 or y0 + h > grid["H"] or x0 + w > grid["W"]:
        raise ValueError(f"region {(y0, x0, h, w)} is empty or leaves the {grid['H']} x {grid['W']} picture")
    rs = [r for r, (_, _, a, b) in enumerate(grid["rows"]) if a < y0 + h and b > y0]
    cs = [c for c, (_, _, a, b) in enumerate(grid["cols"]) if a < x0 + w and b > x0]
    return [(r, c) for r in rs for c in cs]


def select_images(blob, idx) -> bytes:
    """A wire-format 3 / 5 blob -> the ordinary blob of its images ``idx``, in that order (repeats allowed): the same header with
    n = len(idx), their step bytes, their zl / yl length fields and the matching slices of the z and y payloads.  Selecting every
    image in order returns the blob itself.  No device, no model: the stream counts are the header's.  Refused: another version
    (SntcError ERR_UNSUPPORTED -- formats 7 / 8 carry data this function does not cut, format 4 has one latent), a short or long
    blob (ERR_BAD_SHAPE), an empty selection or an index outside the batch (ValueError)."""
    blob = bytes(blob)
    if blob[:4] != MAGIC:
        raise capi.SntcError(capi.ERR_BAD_SHAPE, "not an SNTC bitstream")
    pos = 4 + struct.calcsize(HEAD_V3)
    if len(blob) < 6:
        raise capi.SntcError(capi.ERR_BAD_SHAPE, "bitstream truncated")
    ver = blob[4]
    if ver not in (3, 5):
        raise capi.SntcError(capi.ERR_UNSUPPORTED, f"select_images: bitstream version {ver}; images are cut out of version 3 and 5 files")
    if len(blob) < pos:
        raise capi.SntcError(capi.ERR_BAD_SHAPE, "bitstream truncated")
    fields = list(struct.unpack_from(HEAD_V3, blob, 4))
    n, sz, sy = fields[1], fields[10], fields[11]
    try:
        idx = [int(i) for i in idx]
    except TypeError:
        raise ValueError(f"select_images: idx must be a sequence of image indexes, not {idx!r}") from None
    if not idx:
        raise ValueError("select_images: an empty selection")
    if not all(0 <= i < n for i in idx):
        raise ValueError(f"select_images: index outside the {n} images of the bitstream")
    if len(idx) > MAX_IMAGES:
        raise ValueError(f"select_images: more than {MAX_IMAGES} images")
    steps = b""
    if ver == 5:
        if len(blob) < pos + n:
            raise capi.SntcError(capi.ERR_BAD_SHAPE, "bitstream truncated")
        steps = blob[pos:pos + n]
        pos += n
    if n < 1 or sz < 1 or sy < 1 or len(blob) < pos + 4 * n * (sz + sy):
        raise capi.SntcError(capi.ERR_BAD_SHAPE, "bitstream truncated")
    zl = np.frombuffer(blob, "<u4", n * sz, pos).astype(np.int64).reshape(n, sz)
    yl = np.frombuffer(blob, "<u4", n * sy, pos + 4 * n * sz).astype(np.int64).reshape(n, sy)
    pos += 4 * n * (sz + sy)
    zw, yw = int(zl.sum()), int(yl.sum())
    if len(blob) != pos + 2 * (zw + yw):
        raise capi.SntcError(capi.ERR_BAD_SHAPE, "bitstream truncated")
    if idx == list(range(n)):
        return blob
    zo = np.concatenate([[0], np.cumsum(zl.sum(axis=1))])                 # word offsets of every image's z / y streams
    yo = np.concatenate([[0], np.cumsum(yl.sum(axis=1))])
    fields[1] = len(idx)
    out = [MAGIC, struct.pack(HEAD_V3, *fields), bytes(steps[i] for i in idx) if ver == 5 else b"",
           zl[idx].astype("<u4").tobytes(), yl[idx].astype("<u4").tobytes()]
    out += [blob[pos + 2 * int(zo[i]):pos + 2 * int(zo[i + 1])] for i in idx]
    ybase = pos + 2 * zw
    out += [blob[ybase + 2 * int(yo[i]):ybase + 2 * int(yo[i + 1])] for i in idx]
    return b"".join(out)
