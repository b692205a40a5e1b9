"""Host half of the factorized-prior model's bitstream (entropy_coding.FactorizedCodec, wire format v4): header packing and
parsing are pure functions, and the per-channel integer tables of a deep-factorized prior are valid rANS tables whose
streams the pure-Python restatement of the format codes and decodes.  No GPU."""
import struct

import numpy as np
import pytest

from oracle import rans_np


def noisy_prior(channels, seed=0):
    """deep_factorized_init(C, (3, 3, 3)) with N(0, 0.3) noise on every prior variable: channels of different widths and skews."""
    from shallow_ntc_amd.mshyper.models import deep_factorized_init
    rng = np.random.default_rng(seed)
    pw = deep_factorized_init(channels, (3, 3, 3))
    return {k: (v + 0.3 * rng.standard_normal(v.shape)).astype(np.float32) for k, v in pw.items()}


def latent_shape_of(num_filters):
    """(H, W) -> (C, h, w) as FactorizedCodec.latent_shape computes it for a BLS2017 model: pad to 16, the analysis' out_hw."""
    from shallow_ntc_amd.common.transforms import class_builder
    ana = class_builder.build("BLS2017Analysis", num_filters=num_filters)

    def shape(H, W):
        h, w = ana.out_hw(-(-H // 16) * 16, -(-W // 16) * 16)
        return (ana.out_channels(3), h, w)
    return shape


def test_v4_header_round_trip():
    from shallow_ntc_amd import entropy_coding as ec
    shape = latent_shape_of(64)
    for n, H, W in ((2, 70, 90), (1, 512, 768), (3, 16, 16)):
        c, h, w = shape(H, W)
        assert (c, h, w) == (64, -(-H // 16), -(-W // 16))
        e = c * h * w
        segs = ec._segments(e)
        lanes = ec._lanes(-(-e // segs))
        lens = np.arange(1, n * segs + 1) * 3 + 2 * lanes
        payload = bytes(2 * int(lens.sum()))
        for arith in (0, 1):
            blob = ec.pack_v4(arith, n, H, W, c, h, w, segs, lanes, lens) + payload
            assert blob[:4] == b"SNTC" and blob[4] == 4 and blob[5] == arith
            hd = ec.parse_v4(blob, arith, shape)
            assert (hd["n"], hd["H"], hd["W"], hd["c"], hd["h"], hd["w"], hd["segments"], hd["lanes"]) == (n, H, W, c, h, w, segs, lanes)
            assert hd["lens"].tolist() == lens.tolist() and hd["words"] == int(lens.sum())
            assert hd["pos"] == 4 + struct.calcsize(ec.HEAD_V4) + 4 * n * segs == len(blob) - len(payload)
    with pytest.raises(ec.capi.SntcError):
        ec.pack_v4(0, 2, 70, 90, 64, 5, 6, 1, 8, [20])          # one length for two streams


def test_v4_header_refusals():
    from shallow_ntc_amd import entropy_coding as ec
    shape = latent_shape_of(64)
    n, H, W = 2, 70, 90
    c, h, w = shape(H, W)
    segs, lanes = ec._segments(c * h * w), ec._lanes(c * h * w)
    assert (c, h, w, segs, lanes) == (64, 5, 6, 1, 8)
    lens = np.array([40, 50])
    blob = ec.pack_v4(0, n, H, W, c, h, w, segs, lanes, lens) + bytes(180)
    ec.parse_v4(blob, 0, shape)
    head = list(struct.unpack_from(ec.HEAD_V4, blob, 4))         # ver n H W C h w segments lanes 0
    hsize = struct.calcsize(ec.HEAD_V4)
    lies = dict(n=(1, 3), n_zero=(1, 0), n_huge=(1, 60000), H=(2, 100), H_huge=(2, 100000), W=(3, 40), C=(4, 32), h=(5, 6), w=(6, 5),
                segments=(7, 2), lanes=(8, 64), pad=(9, 1))
    for name, (field, value) in lies.items():
        bad = list(head)
        bad[field] = value
        forged = blob[:4] + struct.pack(ec.HEAD_V4, *bad) + blob[4 + hsize:]
        with pytest.raises(ec.capi.SntcError, match="header|truncated"):
            ec.parse_v4(forged, 0, shape)
        if name in ("C", "h", "w", "segments", "lanes", "H_huge", "n_huge"):
            with pytest.raises(ec.capi.SntcError, match="header"):
                ec.parse_v4(forged, 0, shape)
    for cut in (blob[:-2], blob[:-1], blob[:hsize + 6], blob[:12], blob[:5], blob + b"\0\0"):
        with pytest.raises(ec.capi.SntcError, match="truncated"):
            ec.parse_v4(cut, 0, shape)
    with pytest.raises(ec.capi.SntcError, match="not an SNTC"):
        ec.parse_v4(b"JUNK" + blob[4:], 0, shape)
    # a v3 header (the hyperprior codec's) and a foreign arithmetic tag: unsupported, never decoded
    v3 = b"SNTC" + struct.pack(ec.Codec.HEAD, ec.VERSION, n, H, W, 64, 64, 2, 2, h, w, 1, 1, 8, 8) + bytes(400)
    for other, arith in ((v3, 0), (blob, 1), (blob[:5] + b"\x07" + blob[6:], 0)):
        with pytest.raises(ec.capi.SntcError) as err:
            ec.parse_v4(other, arith, shape)
        assert err.value.code == ec.capi.ERR_UNSUPPORTED
    # a model of another width refuses the same blob
    with pytest.raises(ec.capi.SntcError, match="header"):
        ec.parse_v4(blob, 0, latent_shape_of(256))


def test_tables_of_a_256_channel_prior_code_and_decode():
    from shallow_ntc_amd import entropy_coding as ec
    C = 256
    tabs = ec.factorized_tables(noisy_prior(C), 4)
    assert len(tabs) == C
    for lo, f in tabs:
        assert int(f.sum()) == 65536 and f.min() >= 1 and len(f) >= 2
        assert -2047 <= lo and lo + len(f) - 2 <= 2047                  # real symbols lo .. lo + n - 2, then ESCAPE
    widths = [len(f) for _, f in tabs]
    assert max(widths) > min(widths)                                    # the channels do differ
    assert sum(widths) * 2 + 8 * C < 145 * 1024                         # the encoder's tables fit a CU's LDS ...
    assert 4 * (sum(widths) + 3 * C) > 150 * 1024                       # ... the decoder's packed entries do not
    # values drawn from each channel's own table (so most are in range), plus escapes on both sides
    rng = np.random.default_rng(1)
    P = 9                                                               # 9 x 256 = 2304 symbols: plain Python, keep it small
    vals = np.empty((P, C), np.int64)
    for ch, (lo, f) in enumerate(tabs):
        sym = rng.choice(len(f), size=P, p=np.asarray(f, np.float64) / 65536.0)
        vals[:, ch] = np.where(sym == len(f) - 1, lo - 3, lo + sym)     # a drawn ESCAPE becomes a value just below the table
    vals[0, 3], vals[4, 200], vals[8, 255], vals[2, 0] = 20000, -31000, 32767, -32768
    flat = vals.ravel()
    tids = np.arange(flat.size) % C
    for lanes in (64, 8):
        words = rans_np.encode_stream(flat, tids, tabs, lanes)
        assert rans_np.decode_stream(words, tids, tabs, lanes) == flat.tolist()
        # the cost of the stream against the tables' own code lengths: flushed states in, within a percent
        ideal = 0.0
        for v, t in zip(flat, tids):
            lo, f = tabs[t]
            s = v - lo
            esc = s < 0 or s >= len(f) - 1
            ideal += -np.log2(f[len(f) - 1 if esc else s] / 65536.0) + (16 if esc else 0)
        assert ideal + 16 * lanes < 16 * len(words) <= (ideal + 32 * lanes) * 1.01
