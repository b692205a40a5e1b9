"""Host half of the variable-rate bitstream ("variable rate"): the quantisation-step ladder, wire format v5 (the
v3 header + one signed ladder index per image) and the rate-control rule are pure functions.  No GPU."""
import math
import struct

import numpy as np
import pytest


def shapes(H, W):
    """(C, Cz, hz, wz, h, w) of a 16x / 64x hyperprior model with 320 / 192 channels."""
    return (320, 192, -(-H // 64), -(-W // 64), -(-H // 16), -(-W // 16))


def header_case(n, H, W):
    from shallow_ntc_amd import entropy_coding as ec
    c, cz, hz, wz, h, w = shapes(H, W)
    ez, ey = cz * hz * wz, c * h * w
    sz, sy = ec._segments(ez), ec._segments(ey)
    lz, ly = ec._lanes(-(-ez // sz)), ec._lanes(-(-ey // sy))
    zl = np.arange(1, n * sz + 1) * 3 + 2 * lz
    yl = np.arange(1, n * sy + 1) * 5 + 2 * ly
    payload = bytes(2 * int(zl.sum() + yl.sum()))
    return dict(n=n, H=H, W=W, dims=(c, cz, hz, wz, h, w), sz=sz, sy=sy, lz=lz, ly=ly, zl=zl, yl=yl), payload


def pack(case, steps, arith=0):
    from shallow_ntc_amd import entropy_coding as ec
    return ec.pack_v3(arith, case["n"], case["H"], case["W"], case["dims"], case["sz"], case["sy"], case["lz"], case["ly"], case["zl"],
                      case["yl"], steps)


def test_step_size():
    from shallow_ntc_amd import entropy_coding as ec
    assert (ec.STEP_MIN, ec.STEP_MAX) == (-32, 32)
    assert ec.step_size(0) == 1.0
    ulp = float(np.spacing(np.float32(1.0)))
    for k in range(ec.STEP_MIN, ec.STEP_MAX + 1):
        s, i = ec.step_size(k), ec.step_size(-k)
        assert s == float(np.float32(s)) == float(np.float32(math.exp(k * ec.SCALE_FACTOR)))      # float64, rounded once
        assert abs(s * i - 1.0) <= ulp, (k, s * i)
    for k in (-33, 33, 1000):
        with pytest.raises(ValueError):
            ec.step_size(k)


def test_ladder_identity():
    """sigma_i / step(k) = sigma_(i - k): the symbols of step k are distributed as table i - k describes.  To float64 rounding:
    exp turns the ABSOLUTE rounding error of its argument into a relative one, the arguments here are sums and products of a few
    terms below 16 in magnitude (ulp(8) = 8 eps each), so the two sides agree to a few times 8 eps -- held to 64 eps."""
    from shallow_ntc_amd import entropy_coding as ec
    sigma = lambda i: math.exp(math.log(ec.SCALE_MIN) + ec.SCALE_FACTOR * i)
    for i in range(ec.NUM_SCALES):
        for k in range(ec.STEP_MIN, ec.STEP_MAX + 1):
            got, want = sigma(i) / math.exp(k * ec.SCALE_FACTOR), sigma(i - k)
            assert abs(got / want - 1.0) <= 64 * 2.0 ** -52, (i, k)


@pytest.mark.parametrize("n", [1, 3])
def test_v5_header_round_trip(n):
    from shallow_ntc_amd import entropy_coding as ec
    case, payload = header_case(n, 200, 120)
    steps = [3, -2, 32][:n]
    for arith, prec in ((0, "fp32"), (1, "bf16x3")):
        blob = pack(case, steps, arith) + payload
        assert blob[:4] == b"SNTC" and blob[4] == 5 and blob[5] == arith
        fixed = 4 + struct.calcsize(ec.HEAD_V3)
        assert np.frombuffer(blob, np.int8, n, fixed).tolist() == steps
        hd = ec.parse_v3(blob, prec, shapes)
        assert hd["steps"] == steps
        assert (hd["n"], hd["H"], hd["W"], hd["sz"], hd["sy"], hd["lz"], hd["ly"]) == (n, 200, 120, case["sz"], case["sy"], case["lz"], case["ly"])
        assert (hd["c"], hd["cz"], hd["hz"], hd["wz"], hd["h"], hd["w"]) == case["dims"]
        assert hd["zl"].tolist() == case["zl"].tolist() and hd["yl"].tolist() == case["yl"].tolist()
        assert hd["pos"] == fixed + n + 4 * n * (case["sz"] + case["sy"]) == len(blob) - len(payload)
        # the same fields without steps: the v3 blob is the v5 blob minus the index bytes, version byte 3
        v3 = pack(case, None, arith) + payload
        assert v3[4] == 3 and v3[:4] + v3[5:fixed] == blob[:4] + blob[5:fixed] and v3[fixed:] == blob[fixed + n:]
        assert ec.parse_v3(v3, prec, shapes)["steps"] is None


def test_zero_steps_pack_as_v3():
    from shallow_ntc_amd import entropy_coding as ec
    case, payload = header_case(3, 128, 128)
    assert pack(case, [0, 0, 0]) == pack(case, None)
    assert pack(case, None)[4] == ec.VERSION == 3
    assert pack(case, [0, 1, 0])[4] == ec.VERSION_STEP == 5
    for bad in ([0, 0], [0, 0, 33], [0, -33, 0]):
        with pytest.raises(ValueError):
            pack(case, bad)


def test_v5_refusals():
    from shallow_ntc_amd import entropy_coding as ec
    case, payload = header_case(3, 200, 120)
    blob = pack(case, [3, -2, 32]) + payload
    fixed = 4 + struct.calcsize(ec.HEAD_V3)
    for forged in (33, -33, 127, -128):
        for i in range(3):
            b = bytearray(blob)
            b[fixed + i] = forged & 0xff
            with pytest.raises(ec.capi.SntcError, match="header") as e:
                ec.parse_v3(bytes(b), "fp32", shapes)
            assert e.value.code == ec.capi.ERR_BAD_SHAPE
    lens_end = fixed + 3 + 4 * 3 * (case["sz"] + case["sy"])
    for cut in (fixed - 1, fixed, fixed + 2, fixed + 3, lens_end - 1, len(blob) - 2, len(blob) - 1):
        with pytest.raises(ec.capi.SntcError, match="truncated") as e:
            ec.parse_v3(blob[:cut], "fp32", shapes)
        assert e.value.code == ec.capi.ERR_BAD_SHAPE
    with pytest.raises(ec.capi.SntcError, match="truncated"):
        ec.parse_v3(blob + b"\0\0", "fp32", shapes)
    for ver in (2, 4, 6):
        b = bytearray(blob)
        b[4] = ver
        with pytest.raises(ec.capi.SntcError) as e:
            ec.parse_v3(bytes(b), "fp32", shapes)
        assert e.value.code == ec.capi.ERR_UNSUPPORTED
    with pytest.raises(ec.capi.SntcError) as e:                       # the factorized codec reads v4 only
        ec.parse_v4(blob, 0, lambda H, W: (320, 13, 8))
    assert e.value.code == ec.capi.ERR_UNSUPPORTED


def test_check_steps_and_budgets():
    from shallow_ntc_amd import entropy_coding as ec
    assert ec.check_steps(4, 3) == [4, 4, 4]
    assert ec.check_steps([1, -32, 32], 3) == [1, -32, 32]
    assert ec.check_steps(np.int64(-5), 1) == [-5]
    for bad, n in ((33, 1), (-33, 2), ([1, 2], 3), ([1, 2.5], 2), (1.0, 1), ("3", 1), ([True, 1], 2)):
        with pytest.raises(ValueError):
            ec.check_steps(bad, n)
    assert ec.check_budgets(0.3, 2).tolist() == [0.3, 0.3]
    assert ec.check_budgets([0.3, 1.5], 2).tolist() == [0.3, 1.5]
    for bad, n in (([0.3], 2), (float("nan"), 1), ([[0.3, 0.4]], 2)):
        with pytest.raises(ValueError):
            ec.check_budgets(bad, n)


def test_selection_rule():
    """The finest step that fits, over the whole ladder, from a scripted cost array."""
    from shallow_ntc_amd import entropy_coding as ec
    ladder = list(range(ec.STEP_MIN, ec.STEP_MAX + 1))
    mono = np.array([1000.0 * 0.9 ** (k - ec.STEP_MIN) for k in ladder])          # falls 10 % per step
    wavy = mono.copy()
    wavy[ladder.index(5)] = mono[ladder.index(-3)] + 1.0                           # a row need not be monotone: 5 costs more than -3
    wavy[ladder.index(-10)] = 10.0                                                 # and a fine step may fit where coarser ones do not
    bits = np.stack([mono, mono, mono, wavy, wavy, mono])
    at = lambda row, k: float(row[ladder.index(k)])
    budgets = [0.5 * (at(mono, 7) + at(mono, 6)),          # strictly between bits(7) and bits(6) -> 7
               0.5 * (at(mono, -20) + at(mono, -21)),      # a target ABOVE the model's own rate -> a step below 0
               at(mono, 0),                                # exactly bits(0): fits
               0.5 * (at(mono, -3) + at(mono, -4)),        # wavy: -10 fits (10 bits), and is finer than -3
               5.0,                                        # wavy: below the dip; only the coarse tail of the ladder fits
               at(mono, ec.STEP_MAX) - 1.0]                # unreachable
    rep = ec.select_steps(bits, budgets, ladder)
    assert [r["step_chosen"] for r in rep[:4]] == [7, -20, 0, -10]
    assert rep[3]["bits_predicted"] == 10.0
    k4 = min(k for k in ladder if at(wavy, k) <= 5.0)
    assert rep[4]["step_chosen"] == k4 and k4 > 5
    for r, row, b in zip(rep[:5], bits, budgets):
        assert r["met"] is True and r["bits_predicted"] == at(row, r["step_chosen"]) <= b == r["budget_bits"]
        assert all(at(row, k) > b for k in ladder if k < r["step_chosen"])         # nothing finer fits
    assert rep[5] == dict(step_chosen=ec.STEP_MAX, bits_predicted=at(mono, ec.STEP_MAX), budget_bits=budgets[5], met=False)
    with pytest.raises(ValueError):
        ec.select_steps(bits[:, :-1], budgets, ladder)
