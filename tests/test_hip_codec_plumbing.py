"""The codecs' plumbing on the device (-m gpu): ``ops.fork`` / ``ops.join`` order work across streams both ways, and the decode
front that ``decompress_many`` and ``transcode_many`` share gives what one call per blob gives -- blobs handed over smallest first,
so that the pipeline order (largest first) differs from the argument order --, under ``PIPELINE_BLOBS`` = False, after a refusal in
the middle of the pipeline, and with a layered (format 8) blob among plain ones."""
import pytest
import torch

from test_hip_itinf_bitstream import hyper_model, images  # noqa: F401  (hyper_model: a fixture)

pytestmark = pytest.mark.gpu

BATCHES = ((1, 64, 64), (2, 64, 96), (1, 128, 64))      # 16, 48 and 32 latent positions: pipeline order 1, 2, 0
SHIFTS = [0, 3, [1]]
ELEMS = 64 << 20                                         # floats of the ordering test: a fill of 256 MB takes ~0.1 ms
FILLS = 8


@pytest.mark.parametrize("pooled", (True, False), ids=("pool", "main"))
def test_fork_and_join_order_both_directions(dev, pooled):
    from shallow_ntc_amd import ops
    with torch.cuda.device(dev):
        main, lanes = ops.lanes(2 if pooled else 1, dev)
        lane = lanes[-1]
        assert (lane is main) != pooled and (not pooled or lane is ops.side_streams(2, dev)[1])
        # made on main, read on the lane: without the lane's wait the copy sees an earlier fill
        a = torch.empty(ELEMS, dtype=torch.float32, device=dev)
        for v in range(1, FILLS + 1):
            a.fill_(float(v))
        with ops.fork(main, lane, reads=(a,)):
            b = a.clone()
        ops.join(main, lane, made=(b,))
        forward = bool((b == float(FILLS)).all())
        del a
        # made on the lane, consumed on main: without main's wait the copy sees an earlier fill
        with ops.fork(main, lane):
            c = torch.empty(ELEMS, dtype=torch.float32, device=dev)
            for v in range(1, FILLS + 1):
                c.fill_(float(-v))
        ops.join(main, lane, made=(c,))
        d = c.clone()
        backward = bool((d == float(-FILLS)).all())
        assert forward and backward


@pytest.fixture(scope="module")
def case(dev, hyper_model):
    """The three blobs, smallest first, and what one call per blob gives: computed once, never modified."""
    xs = [images(n, h, w, dev, seed=31 + i) for i, (n, h, w) in enumerate(BATCHES)]
    blobs = [hyper_model.compress(x) for x in xs]
    layered = hyper_model.compress(xs[1], max_error=1)
    return dict(xs=xs, blobs=blobs, pixels=[hyper_model.decompress(b).clone() for b in blobs],
                moved=[hyper_model.transcode(b, shift=s) for b, s in zip(blobs, SHIFTS)],
                layered=layered, layered_pixels=hyper_model.decompress(layered).clone())


def same_pixels(got, want):
    return len(got) == len(want) and all(g.shape == w.shape and torch.equal(g, w) for g, w in zip(got, want))


def test_many_equals_one_call_per_blob(hyper_model, case):
    assert same_pixels(hyper_model.decompress_many(case["blobs"]), case["pixels"])
    assert hyper_model.transcode_many(case["blobs"], shift=SHIFTS) == case["moved"]
    assert [b[4] for b in case["moved"]] == [3, 5, 5]            # the shifts took: format 3 stays, 3 and [1] move to format 5


def test_two_phase_schedule_gives_the_same_pixels(hyper_model, case, monkeypatch):
    from shallow_ntc_amd import entropy_coding as ec
    monkeypatch.setattr(ec, "PIPELINE_BLOBS", False)
    assert same_pixels(hyper_model.decompress_many(case["blobs"]), case["pixels"])
    assert hyper_model.transcode_many(case["blobs"], shift=SHIFTS) == case["moved"]


class WrongShapeOnce:
    """The model's hyper-synthesis, except that call number ``at`` returns one channel too few."""

    def __init__(self, real, at):
        self.real, self.at, self.calls = real, at, 0

    def __getattr__(self, name):
        return getattr(self.real, name)

    def __call__(self, x):
        out = self.real(x)
        self.calls += 1
        return out[..., :-1] if self.calls - 1 == self.at else out


def test_a_refusal_inside_the_pipeline_leaves_the_device_usable(hyper_model, case, monkeypatch):
    """The second blob in pipeline order fails its shape check while the first one's latents decode on their lane from the one
    upload buffer: the error leaves, and the next call -- which allocates the same sizes -- decodes the right pixels."""
    from shallow_ntc_amd import _capi as capi
    patched = WrongShapeOnce(hyper_model._hyper_synthesis, 1)
    monkeypatch.setattr(hyper_model, "_hyper_synthesis", patched)
    with pytest.raises(capi.SntcError, match="hyper-synthesis output"):
        hyper_model.decompress_many(case["blobs"])
    assert patched.calls == 2
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert same_pixels(hyper_model.decompress_many(case["blobs"]), case["pixels"])


def test_a_layered_blob_among_plain_ones(hyper_model, case):
    blobs = [case["blobs"][0], case["layered"], case["blobs"][2]]
    want = [case["pixels"][0], case["layered_pixels"], case["pixels"][2]]
    assert same_pixels(hyper_model.decompress_many(blobs), want)
    assert not torch.equal(case["layered_pixels"], case["pixels"][1])          # the layer did change pixels
