"""Host half of the codecs' plumbing (shallow-ntc_amd/entropy_coding.py, ops.py): the one upload packer, the slicing of the one
finisher and fork / join on the caller's own stream.  CPU tensors, no device."""
import itertools

import numpy as np
import pytest
import torch

I64, I16, U8 = np.int64, np.int16, np.uint8


def arr(dtype, n, seed):
    rng = np.random.default_rng(seed)
    info = np.iinfo(dtype)
    return rng.integers(info.min, info.max, size=n, endpoint=True, dtype=dtype)


def check_pack(arrays):
    from shallow_ntc_amd import entropy_coding as ec
    up, views = ec.pack_upload(arrays, "cpu")
    assert up.dtype == torch.uint8 and up.dim() == 1 and len(views) == len(arrays)
    assert up.numel() <= sum(a.nbytes for a in arrays) + 7 * len(arrays)
    spans = []
    for a, v in zip(arrays, views):
        assert v.dtype == torch.from_numpy(np.empty(0, a.dtype)).dtype and tuple(v.shape) == (a.size,)
        assert np.array_equal(v.numpy(), a.reshape(-1))
        assert v.untyped_storage().data_ptr() == up.untyped_storage().data_ptr()          # a view of the one buffer ...
        at = v.storage_offset() * v.element_size()
        assert at % a.itemsize == 0 and at + a.nbytes <= up.numel()                       # ... aligned, inside it ...
        assert up[at:at + a.nbytes].numpy().tobytes() == a.tobytes()                      # ... holding the array's bytes there
        spans.append((at, at + a.nbytes))
    assert all(e0 <= s1 for (_, e0), (s1, _) in zip(sorted(spans), sorted(spans)[1:]))    # no two views overlap


@pytest.mark.parametrize("order", list(itertools.permutations((I64, I16, U8))), ids=lambda o: "-".join(np.dtype(d).name for d in o))
def test_pack_upload_in_every_order(order):
    for sizes in ((5, 7, 3), (1, 1, 1), (0, 3, 0), (2, 0, 5), (0, 0, 0), (4, 1, 9)):
        check_pack([arr(d, n, 10 * i + n) for i, (d, n) in enumerate(zip(order, sizes))])


@pytest.mark.parametrize("odd", (1, 3, 7))
def test_pack_upload_pads_after_an_odd_run_of_words(odd):
    check_pack([arr(I16, odd, 1), arr(I64, 4, 2)])
    check_pack([arr(U8, odd, 3), arr(I16, odd, 4), arr(I64, 2, 5), arr(U8, 1, 6), arr(I64, 0, 7), arr(I16, 2, 8)])


def test_pack_upload_of_a_single_array_and_of_a_matrix():
    from shallow_ntc_amd import entropy_coding as ec
    for a in (arr(I64, 6, 1), arr(I16, 1, 2), arr(U8, 0, 3)):
        check_pack([a])
    choice = arr(U8, 48, 4).reshape(2, 24)                        # the residual layer's choice bytes: flattened in order
    check_pack([arr(I64, 3, 5), choice])
    assert ec.pack_upload([], "cpu")[1] == []


def test_pack_upload_takes_the_words_of_a_blob_where_they_lie():
    blob = b"\x01" + arr(I16, 5, 9).tobytes()                       # np.frombuffer at an odd offset of a bytes object, "<i2"
    check_pack([np.arange(3, dtype=I64), np.frombuffer(blob, "<i2", 5, 1)])


# ------------------------------------------------------------------ the finisher ---------------------------------------------
def host_compact(scratch, lens, lens_h):
    """What ``rans_encode_finish`` computes (sntc_rans_compact): row i's first lens_h[i] words, back to back."""
    assert np.array_equal(lens.numpy(), lens_h)
    return torch.cat([scratch[i, :int(n)] for i, n in enumerate(lens_h)] + [scratch.new_empty(0)])


def group(streams, cap, seed, lens=None):
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, cap, size=streams, endpoint=True) if lens is None else np.asarray(lens)
    return torch.from_numpy(arr(I16, streams * cap, seed).reshape(streams, cap)), torch.from_numpy(lens.astype(np.int32))


@pytest.mark.parametrize("shape", ([1], [2], [2, 1, 2], [1, 1, 1]), ids=str)
def test_finish_streams_slices_per_blob_and_group(shape, monkeypatch):
    from shallow_ntc_amd import entropy_coding as ec
    calls = []
    monkeypatch.setattr(ec, "rans_encode_finish", host_compact)
    monkeypatch.setattr(ec.ops, "check_conv_status", lambda: calls.append("checked"))
    seeds = itertools.count(1)
    jobs = [[group(2 + s % 3, 8 + s, s) for s in itertools.islice(seeds, groups)] for groups in shape]
    jobs[-1][-1] = group(3, 9, 99, lens=[4, 0, 9])                 # one stream of length 0, one that fills its row
    got = ec.finish_streams(jobs)
    assert calls == ["checked"] and [len(g) for g in got] == shape
    for job, done in zip(jobs, got):
        for (scratch, lens), (lens_h, words) in zip(job, done):
            want_lens = lens.cpu().numpy().astype(np.int64)
            assert lens_h.dtype == np.int64 and np.array_equal(lens_h, want_lens)
            want = host_compact(scratch, lens, want_lens).cpu().numpy()
            assert words.dtype == np.int16 and np.array_equal(words, want)


def test_finish_streams_reads_back_twice(monkeypatch):
    """All lengths in one tensor, all payloads in another: what goes to the host is two tensors whatever the blob count."""
    from shallow_ntc_amd import entropy_coding as ec
    monkeypatch.setattr(ec, "rans_encode_finish", host_compact)
    monkeypatch.setattr(ec.ops, "check_conv_status", lambda: None)
    reads = []
    real = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **k: (reads.append(tuple(t.shape)), real(t, *a, **k))[1])
    jobs = [[group(2, 8, 1), group(3, 8, 2)], [group(1, 8, 3)]]
    total = sum(int(lens.sum()) for job in jobs for _, lens in job)
    ec.finish_streams(jobs)
    assert reads == [(6,), (total,)]


# ------------------------------------------------------------------ fork / join ------------------------------------------------
class Untouchable:
    """A stream no method of which may be called: every attribute access raises."""

    def __getattribute__(self, name):
        raise AssertionError(f"stream.{name} touched although the lane is the caller's stream")


def test_fork_and_join_on_the_callers_own_stream_only_run_the_body():
    from shallow_ntc_amd import ops
    main = Untouchable()
    ran = []
    with ops.fork(main, main, reads=(Untouchable(),)):
        ran.append(1)
    assert ops.join(main, main, made=(Untouchable(),)) is None and ran == [1]
    with pytest.raises(KeyError):                                    # an error in the body leaves as it is
        with ops.fork(main, main):
            raise KeyError("body")
