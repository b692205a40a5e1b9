"""Bitstream from SGA-refined latents (-m gpu): the exact coded cost kernel against its numpy restatement (integer equality),
the file's payload against that cost, ``compress_latents`` / ``coded_cost`` / ``compress(x, itinf=...)`` on both model families."""
import numpy as np
import pytest
import torch

from oracle import rans_np
from test_hip_bitstream import RANS_LDS_LIMIT
from test_rans_cost_host import noisy_prior_tables, np_cost, ref_cost_table

pytestmark = pytest.mark.gpu

N = 3
# 1, a wave +- 1, one workgroup's span +- 1 on both load paths (1024 elements per pass; 4096 where E % 4 == 0), many workgroups
SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 70001]
ITINF = dict(steps=8, seed=3, check_every=4)


def make_case(E, ntables=64, seed=0):
    """[3, E] values / table ids.  Image 0: ids over every table, values as in test_start_tables_do_not_change_a_decoded_value
    plus runs of escapes on both sides of the tables and beyond +-32768; image 1: all in the widest normal table; image 2:
    every value escapes."""
    from shallow_ntc_amd import entropy_coding as ec
    rng = np.random.default_rng(seed + E)
    tids = rng.integers(0, ntables, size=(N, E)).astype(np.int16)
    tids[1] = 63
    sig = np.array([0.11 * np.exp(ec.SCALE_FACTOR * min(k, 63)) * (1 if k < 64 else 40) for k in range(ntables)])
    vals = np.rint(rng.standard_normal((N, E)) * sig[tids] * np.where(rng.random((N, E)) < 0.2, 3.5, 1.0)).astype(np.int32)
    k = min(40, E)
    vals[0, :k] = rng.integers(-30000, 30000, k)
    vals[0, E - min(8, E):] = np.resize(np.array([40000, -40000, 32768, -32769, 32767, -32768, 100000, -100000], np.int32), min(8, E))
    vals[2] = np.where(rng.random(E) < 0.5, 1, -1) * rng.integers(5000, 45000, E)
    return vals, tids


@pytest.fixture(scope="module")
def normal(dev):
    from shallow_ntc_amd import entropy_coding as ec
    tabs = ec.normal_tables()
    return tabs, ec.DeviceTables(tabs, dev), ref_cost_table(tabs)


@pytest.fixture(scope="module")
def cases(normal):
    tabs, _, q = normal
    out = {}
    for E in SIZES:
        vals, tids = make_case(E)
        out[E] = (vals, tids, np_cost(vals, tids, tabs, q))
    return out


def dv(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.parametrize("E", SIZES)
def test_rans_cost_is_the_numpy_sum(E, dev, normal, cases):
    from shallow_ntc_amd import entropy_coding as ec
    tabs, dt, q = normal
    np.testing.assert_array_equal(dt.cost_q.cpu().numpy().view(np.uint32).astype(np.uint64), q)
    vals, tids, want = cases[E]
    got = ec.rans_cost(dv(vals, dev), dv(tids, dev), dt)
    assert got.dtype == torch.int64 and tuple(got.shape) == (N,)
    assert got.cpu().numpy().tolist() == want.tolist()
    # every element of image 2 escapes: at least the 16 raw bits + 16 - log2(escape frequency) each
    assert want[2] >= E * 16 * 65536
    # a view that starts 4 bytes into the allocation: the scalar load path on an E that would take the vector path
    if E % 4 == 0:
        pad_v = torch.cat([torch.zeros(1, dtype=torch.int32, device=dev), dv(vals, dev).flatten()])[1:].view(N, E)
        assert ec.rans_cost(pad_v, dv(tids, dev), dt).cpu().numpy().tolist() == want.tolist()


def big_table_set():
    """The set of test_table_set_beyond_the_lds_limit: the 64 normal tables + 20 wide two-sided geometric ones."""
    from shallow_ntc_amd import entropy_coding as ec
    extra = []
    for k in range(20):
        half = 1500 + 100 * k
        v = np.arange(-half, half + 1)
        extra.append((-half, ec.quantize_pmf(np.exp(-np.abs(v) / (50.0 + 40 * k)), 2.0 ** -12)))
    big = ec.normal_tables() + extra
    assert 8 * len(big) + 4 * ((sum(len(f) for _, f in big) + 1) // 2) > RANS_LDS_LIMIT
    return big


def test_rans_cost_with_tables_beyond_the_lds_limit(dev):
    """Descriptors and costs read from global memory: ids over all 84 tables, the same exact sums."""
    from shallow_ntc_amd import entropy_coding as ec
    big = big_table_set()
    db, q = ec.DeviceTables(big, dev), ref_cost_table(big)
    for E in (65, 4096, 70001):
        vals, tids = make_case(E, ntables=len(big), seed=7)
        assert ec.rans_cost(dv(vals, dev), dv(tids, dev), db).cpu().numpy().tolist() == np_cost(vals, tids, big, q).tolist()


def test_rans_cost_through_the_channel_tables(dev):
    """The factorized-prior path: float latents -> round_to_int + channel_table_ids -> rans_cost, one table per channel."""
    from shallow_ntc_amd import entropy_coding as ec
    tabs = noisy_prior_tables(16, seed=3)
    dt = ec.DeviceTables(tabs, dev)
    rng = np.random.default_rng(9)
    for h, w in ((1, 1), (5, 13), (33, 67)):
        y = (rng.standard_normal((N, h, w, 16)) * 6).astype(np.float32)
        y[1] *= 40                                              # mostly escapes
        y[2, 0, 0, :4] = [40000.5, -40000.5, 0.5, 1.5]          # beyond 16 bits; ties round to even
        yd = dv(y, dev)
        yi, tid = ec.round_to_int(yd), ec.channel_table_ids(yd.shape, dev)
        got = ec.rans_cost(yi, tid, dt).cpu().numpy()
        want = np_cost(np.rint(y).astype(np.int64).reshape(N, -1), np.tile(np.arange(16), (N, h * w)), tabs)
        assert got.tolist() == want.tolist()


def test_file_payload_against_the_cost(dev, normal, cases, monkeypatch):
    """Per stream, payload bits = cost / 65536 + 32 per lane (the flushed states) + the coder's slack: what the 32-bit states
    round away at every renormalisation, minus the up to 16 bits per lane a final state holds less than its 32.  No closed form;
    the bar is twice the largest |gap| the pure-Python restatement of the format shows on these inputs, at least 16 bits per
    lane.  (The restatement recomputes a table's cdf per element; the cdf is memoised here, the words are the same.)
    Measured: the largest |gap| is 404 bits (the 70 001-element all-escape stream, 64 lanes); -128 ... +64 on the others."""
    from shallow_ntc_amd import entropy_coding as ec
    tabs, dt, _ = normal
    memo = {}
    plain = rans_np._cdf
    monkeypatch.setattr(rans_np, "_cdf", lambda f: memo.setdefault(id(f), plain(f)))
    ltabs = [(lo, [int(c) for c in f]) for lo, f in tabs]
    rows = []
    for E in SIZES:
        vals, tids, cost = cases[E]
        lanes = ec._lanes(E)
        payload, lens = ec.rans_encode(dv(vals, dev), dv(tids, dev), dt)
        assert len(lens) == N                                   # one stream per image at these sizes
        for b in range(N):
            ideal = cost[b] / 65536.0 + 32 * lanes
            ref_bits = 16 * len(rans_np.encode_stream(vals[b], tids[b].astype(np.int64) & 0xFFFF, ltabs, lanes))
            rows.append((E, b, lanes, 16 * int(lens[b]) - ideal, ref_bits - ideal))
    worst = max(abs(r[4]) for r in rows)
    print(f"\nrANS slack: largest |payload - (cost + 32 L)| of the restatement = {worst:.2f} bits; per stream (E, image, lanes, gpu, ref):")
    for r in rows:
        print("  E=%d image=%d lanes=%d gpu=%.2f ref=%.2f" % r)
    for E, b, lanes, gap, _ in rows:
        assert abs(gap) <= max(2 * worst, 16 * lanes), (E, b, gap, worst)


# -- codec ---------------------------------------------------------------------------------------------------------------
def images(n, h, w, dev, seed=21):
    from shallow_ntc_amd.common import data_lib
    return torch.from_numpy(data_lib.normalize_image(data_lib.synthetic_images(n, h, w, seed=seed))).to(dev)


def _spread_scales(model):
    """Random weights leave every scale at its floor; spread the scale biases as test_codec_round_trip_and_rate does."""
    w = dict(model.get_weights())
    b = w["hyper_synthesis/layer_2/bias"].copy()
    b[320:] = np.random.default_rng(0).uniform(-1.0, 2.5, size=320)
    w["hyper_synthesis/layer_2/bias"] = b.astype(np.float32)
    model.set_weights(w)
    return model


@pytest.fixture(scope="module")
def hyper_model(dev):
    from shallow_ntc_amd.mshyper import configs
    from shallow_ntc_amd.mshyper.models import Model
    return _spread_scales(Model(device=dev, **{**configs.two_layer_syn(rd_lambda=0.02), **configs.itinf()}))


@pytest.fixture(scope="module")
def fact_model(dev):
    from shallow_ntc_amd.factorized.models import Model
    from shallow_ntc_amd.mshyper import configs
    return Model(device=dev, **{**configs.bls2017(rd_lambda=0.02), **configs.itinf()})


def payload_bits(model, blob):
    """Per image, the bits of its streams in the blob (header and length fields excluded)."""
    hd = model._get_codec()._parse(blob)
    if model.factorized:
        return 16.0 * hd["lens"].reshape(hd["n"], -1).sum(axis=1), hd
    return 16.0 * (hd["zl"].reshape(hd["n"], -1).sum(axis=1) + hd["yl"].reshape(hd["n"], -1).sum(axis=1)), hd


def image_words(model, blob, i):
    """The stream lengths and words of image i in a blob."""
    hd = model._get_codec()._parse(blob)
    words = np.frombuffer(blob, "<u2", offset=hd["pos"])
    out = []
    base = 0
    for key in (("lens",) if model.factorized else ("zl", "yl")):
        lens = hd[key].reshape(hd["n"], -1)
        off = base + int(lens[:i].sum())
        out.append((lens[i].tolist(), words[off:off + int(lens[i].sum())].tolist()))
        base += int(lens.sum())
    return out


def pixels_of(model, latents, hw):
    """The established decode path on given latents: round z, hyper-synthesis, symbols = round(y - mu), ``decode``."""
    from shallow_ntc_amd import entropy_coding as ec
    from shallow_ntc_amd import ops
    locs = [rv.loc for rv in latents.uq]
    if model.factorized:
        return model.decode(ec.int_to_float(ec.round_to_int(locs[0])), None, hw)
    z_hat = ec.int_to_float(ec.round_to_int(locs[0]))
    sym = ops.entropy_scale_normal(locs[1], model._hyper_synthesis(z_hat), want_symbols=True)[2]
    return model.decode(z_hat, sym, hw)


def slack_bar(model, hd):
    """The bar of test_file_payload_against_the_cost per image: 16 bits per flushed lane state of its streams (twice the
    restatement's largest gap, DESIGN.md 4.7, is below that for every lane count)."""
    if model.factorized:
        return 16.0 * hd["segments"] * hd["lanes"]
    return 16.0 * (hd["sz"] * hd["lz"] + hd["sy"] * hd["ly"])


def flushed_bits(model, hd):
    return 2.0 * slack_bar(model, hd)


CODEC_CASES = [("hyper", 2, 128, 128), ("hyper", 1, 200, 120), ("fact", 2, 64, 96)]


@pytest.mark.parametrize("kind,n,h,w", CODEC_CASES, ids=["hyper-2x128x128", "hyper-1x200x120", "fact-2x64x96"])
def test_compress_with_itinf(kind, n, h, w, dev, hyper_model, fact_model):
    model = hyper_model if kind == "hyper" else fact_model
    x = images(n, h, w, dev)
    codec = model._get_codec()
    # today's path, byte for byte: itinf=None, and compress_latents on the encoder's latents
    plain = model.compress(x)
    assert model.compress(x, itinf=None) == plain
    lat = model.infer_latent_rvs(x)
    assert codec.compress_latents(*[rv.loc for rv in lat.uq], (h, w)) == plain
    assert model.compress_many([x]) == [plain]
    # coded_cost of the encoder's latents against the file
    cost = model.coded_cost(x)
    bits, hd = payload_bits(model, plain)
    for i in range(n):
        assert abs(bits[i] - (cost["bits"][i] + flushed_bits(model, hd))) <= slack_bar(model, hd), (i, bits[i], cost["bits"][i])
    px0 = model.decompress(plain)
    sse0 = ((px0.cpu().numpy().astype(np.int64) - np.rint((x.cpu().numpy().astype(np.float64) + 0.5) * 255)) ** 2).reshape(n, -1).sum(axis=1)
    assert cost["sse"].tolist() == sse0.tolist()
    np.testing.assert_allclose(cost["J"], cost["bits"] / (h * w) + 0.02 * sse0 / (h * w * 3), rtol=1e-12)
    # SGA, then the best candidate per image by exact coded cost
    blob = model.compress(x, itinf=ITINF)
    rep = model.last_compress_report
    assert len(rep) == n and model.global_step == ITINF["steps"]
    print()
    for i, r in enumerate(rep):
        print(f"{kind} {n}x{h}x{w} image {i}: step {r['step_chosen']}  J {r['J_start']:.6f} -> {r['J_chosen']:.6f} "
              f"(gain {r['J_start'] - r['J_chosen']:.6f})  bits {r['bits_start']:.1f} -> {r['bits_chosen']:.1f}")
        assert r["J_chosen"] <= r["J_start"] and r["step_chosen"] in (0, 4, 8)
        assert r["J_start"] == cost["J"][i] and r["bits_start"] == cost["bits"][i]
        assert (r["step_chosen"] == 0) == (r["J_chosen"] == r["J_start"])
    chosen = model.last_compress_latents
    assert torch.equal(model.decompress(blob), pixels_of(model, chosen, (h, w)))
    after = model.coded_cost(x, chosen)
    assert after["J"].tolist() == [r["J_chosen"] for r in rep] and after["bits"].tolist() == [r["bits_chosen"] for r in rep]
    bits, hd = payload_bits(model, blob)
    for i in range(n):
        assert abs(bits[i] - (after["bits"][i] + flushed_bits(model, hd))) <= slack_bar(model, hd)
        if rep[i]["step_chosen"] == 0:                          # the encoder's own latents were kept: the plain file's streams
            assert image_words(model, blob, i) == image_words(model, plain, i)
    # An image's SGA draw is keyed by its element index in the BATCH and its gradient is that of the batch mean, so an image
    # refined alone walks another path than inside a batch: its bytes are compared with those of ITS chosen latents coded
    # alone -- the per-image selection must not have mixed images, and the coder is batch-invariant.
    if n > 1:
        for i in range(n):
            alone = codec.compress_latents(*[rv.loc[i:i + 1].contiguous() for rv in chosen.uq], (h, w))
            assert image_words(model, alone, 0) == image_words(model, blob, i)


def test_selection_keeps_each_images_best_candidate(dev, hyper_model, monkeypatch):
    """A scripted J per candidate (image 0 best at step 4, image 1 at step 0, image 2 at step 8): each image's coded latents
    are its own at the scripted step, whatever the other images chose."""
    model = hyper_model
    x = images(3, 64, 64, dev, seed=5)
    script = iter([[5.0, 1.0, 5.0], [3.0, 2.0, 4.5], [3.0, 1.5, 4.0]])
    real_cost, real_step, snaps = model.coded_cost, model.itinf_train_step, {}

    def cost(xx, latent_rvs=None):
        c = real_cost(xx, latent_rvs)
        c["J"] = np.array(next(script))
        snaps[model.global_step] = [rv.loc.clone() for rv in latent_rvs.uq]
        return c

    monkeypatch.setattr(model, "coded_cost", cost)
    blob = model.compress(x, itinf=ITINF)
    monkeypatch.undo()
    rep = model.last_compress_report
    assert [r["step_chosen"] for r in rep] == [4, 0, 8] and [r["J_chosen"] for r in rep] == [3.0, 1.0, 4.0]
    assert sorted(snaps) == [0, 4, 8]
    for i, step in enumerate((4, 0, 8)):
        for kept, snap in zip(model.last_compress_latents.uq, snaps[step]):
            assert torch.equal(kept.loc[i], snap[i])
    assert not torch.equal(snaps[0][1], snaps[8][1])            # SGA moved the latents at all
    assert torch.equal(model.decompress(blob), pixels_of(model, model.last_compress_latents, (64, 64)))


def test_ms_ssim_cost_and_refusals(dev, monkeypatch):
    """distortion="ms_ssim" on 64 x 96 (both sides < 160: single-scale SSIM): J = bits / (H W) + lambda (1 - q) with q the SSIM
    of the decoded pixels; an 8 x 8 image is refused before anything runs.  The other refusals of compress(itinf=...)."""
    from shallow_ntc_amd import ops
    from shallow_ntc_amd.mshyper import configs
    from shallow_ntc_amd.mshyper.models import Model
    from test_hip_sga import TC
    model = Model(device=dev, distortion="ms_ssim", **{**configs.two_layer_syn(rd_lambda=8.0), **configs.itinf()})
    x = images(2, 64, 96, dev, seed=4)
    blob = model.compress(x, itinf=ITINF)
    rep = model.last_compress_report
    after = model.coded_cost(x, model.last_compress_latents)
    px = model.decompress(blob)
    q = ops.image_quality(ops.pixels_float(x, 64, 96), px.to(torch.float32), 255.0)
    np.testing.assert_array_equal(after["msssim"], q)
    np.testing.assert_array_equal(after["D"], 1.0 - q)
    np.testing.assert_allclose(after["J"], after["bits"] / (64 * 96) + 8.0 * (1.0 - q), rtol=1e-12)
    for i, r in enumerate(rep):
        print(f"ms_ssim image {i}: step {r['step_chosen']}  J {r['J_start']:.6f} -> {r['J_chosen']:.6f}")
        assert r["J_chosen"] <= r["J_start"] and r["J_chosen"] == after["J"][i]
    tiny = images(1, 8, 8, dev)
    launches, analysis = [], model.infer_latent_rvs
    monkeypatch.setattr(model, "infer_latent_rvs", lambda *a, **k: launches.append(1) or analysis(*a, **k))
    with pytest.raises(ValueError, match="SSIM"):
        model.compress(tiny, itinf=ITINF)
    with pytest.raises(ValueError, match="SSIM"):
        model.coded_cost(tiny)
    assert not launches                                         # refused before the analysis ran
    x64 = images(1, 64, 64, dev)
    unoise = Model(device=dev, rd_lambda=0.02, transform_config=TC)
    with pytest.raises(NotImplementedError, match="sga"):
        unoise.compress(x64, itinf=ITINF)
    split = Model(device=dev, rd_lambda=0.02, transform_config=TC, precision="bf16x3", **configs.itinf())
    with pytest.raises(NotImplementedError, match="fp32"):
        split.compress(x64, itinf=ITINF)
    assert unoise.compress(x64, itinf=None) == unoise.compress(x64)
