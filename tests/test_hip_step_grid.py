"""The three quantisation grids launch for launch (-m gpu): the library calls of compress_latents / decompress / latents_cost /
one SGA step on a unit, a per-image and a per-position grid, and of the routed cases (all-zero offsets, offsets constant per
image, ``decompress_many`` of the three blobs, a per-image ``rd_lambda`` at step 0), against the sequences recorded on the commit
before ``entropy_coding.StepGrid`` (tests/golden/step_grid_calls.json: names only).  A pull request that changes launches on
purpose regenerates the file with ``record_calls`` and says so."""
import json
from pathlib import Path

import numpy as np
import pytest

from test_hip_itinf_bitstream import hyper_model, images  # noqa: F401

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "step_grid_calls.json"
N, H, W = 2, 64, 64                     # 4 x 4 latent positions: the smallest on which a map varies inside an image
IMAGE_STEPS = [3, -3]
RD_LAMBDAS = [0.01, 0.03]


def grid_arguments():
    """kind -> the ``step`` / ``step_offsets`` keywords that select it."""
    varying = np.tile(np.array([0, 3, -3, 0], np.int8), (N, 4, 1))
    varying[1] = varying[1].T
    constant = np.broadcast_to(np.array(IMAGE_STEPS, np.int8)[:, None, None], (N, 4, 4)).copy()
    return dict(unit={}, image=dict(step=IMAGE_STEPS), map=dict(step_offsets=varying),
                zero_offsets=dict(step_offsets=np.zeros((N, 4, 4), np.int8)), constant_offsets=dict(step_offsets=constant))


def record_calls(model, x, monkeypatch):
    """Every case's ``sntc_*`` names in call order -> dict(case -> [names]).  Each case runs once unrecorded first, so that what a
    first use adds (plans, tuning, cached tables) is in neither the recording nor the file."""
    from shallow_ntc_amd import _capi as capi
    names, plain = [], capi.call

    def spy(name, *args):
        names.append(name)
        return plain(name, *args)

    def recorded(fn):
        fn()
        del names[:]
        out = fn()
        return list(names), out

    monkeypatch.setattr(capi, "call", spy)
    codec = model._get_codec()
    lat = model.infer_latent_rvs(x)
    z, y = (rv.loc.contiguous() for rv in lat.uq)
    calls, blobs = {}, {}
    for kind, kw in grid_arguments().items():
        calls[f"{kind}/compress_latents"], blob = recorded(lambda: codec.compress_latents(z, y, (H, W), **kw))
        calls[f"{kind}/decompress"], _ = recorded(lambda: codec.decompress(blob))
        calls[f"{kind}/latents_cost"], _ = recorded(lambda: codec.latents_cost(z, y, x, **kw))
        blobs[kind] = blob
    calls["decompress_many"], _ = recorded(lambda: codec.decompress_many([blobs[k] for k in ("unit", "image", "map")]))

    def sga(**kw):
        model.initialize_itinf(x, **kw)
        model.itinf_train_step(x, seed=0, fetch=False)

    for kind, kw in grid_arguments().items():
        calls[f"{kind}/itinf"], _ = recorded(lambda: sga(**kw))
    calls["rd_lambda/itinf"], _ = recorded(lambda: sga(step=0, rd_lambda=RD_LAMBDAS))
    monkeypatch.setattr(capi, "call", plain)
    return calls, blobs


def test_library_calls_are_those_of_before(dev, hyper_model, monkeypatch):
    want = json.loads(GOLDEN.read_text())
    x = images(N, H, W, dev)
    got, blobs = record_calls(hyper_model, x, monkeypatch)
    assert [blobs[k][4] for k in ("unit", "image", "map", "zero_offsets", "constant_offsets")] == [3, 5, 7, 3, 5]
    assert set(got) == set(want)
    for case in sorted(want):
        print(f"{case}: {len(got[case])} calls")
        assert got[case] == want[case], case
    # the routed cases take the route of the grid they resolve to -- in the file, so in the code
    for op in ("compress_latents", "decompress", "latents_cost", "itinf"):
        assert want[f"zero_offsets/{op}"] == want[f"unit/{op}"] and want[f"constant_offsets/{op}"] == want[f"image/{op}"]
    # a per-image lambda at step 0 takes the per-image SGA kernels; every kind its own
    for case, fwd in (("unit/itinf", "sntc_sga_normal_fwd"), ("image/itinf", "sntc_sga_normal_step_fwd"),
                      ("map/itinf", "sntc_sga_normal_step_map_fwd"), ("rd_lambda/itinf", "sntc_sga_normal_step_fwd")):
        assert [n for n in want[case] if n.startswith("sntc_sga_normal")] == [fwd, fwd.replace("_fwd", "_bwd")]
    for kind, sym, deq in (("image", "sntc_step_symbols", "sntc_dequant_step"), ("map", "sntc_step_map_symbols", "sntc_dequant_step_map")):
        assert sym in want[f"{kind}/compress_latents"] and deq in want[f"{kind}/decompress"] and deq in want[f"{kind}/latents_cost"]
    for deq in ("sntc_dequant_step", "sntc_dequant_step_map"):
        assert want["decompress_many"].count(deq) == 1
