"""bench.py --dump-outputs on the host: file names, dtype, the byte budget, and a sample that is the same on every run."""
import numpy as np
import torch

import bench


def test_dump_outputs_budget_and_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "np", np)          # main() imports numpy / torch into the module in the worker processes
    monkeypatch.setattr(bench, "torch", torch)
    g = torch.Generator().manual_seed(0)
    outs = [torch.randint(0, 256, (6, 768, 512, 3), generator=g, dtype=torch.uint8),       # the Kodak-shaped set's two batches
            torch.randint(0, 256, (18, 512, 768, 3), generator=g, dtype=torch.uint8)]
    for d in ("a", "b"):
        bench.dump_outputs(outs, tmp_path / d)
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == ["pixels0_6x768x512.npy", "pixels1_18x512x768_sample.npy"]
    assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) < 64e6
    whole = np.load(tmp_path / "a" / names[0])
    assert whole.dtype == np.float32 and np.array_equal(whole, outs[0].numpy())
    sa, sb = (np.load(tmp_path / d / names[1]) for d in ("a", "b"))
    assert sa.dtype == np.float32 and np.array_equal(sa, sb)
    assert sa.size == bench.DUMP_BUDGET_BYTES // 4 - outs[0].numel()       # the smaller batch's unused share goes to the larger
    assert np.array_equal(np.bincount(sa.astype(np.int64), minlength=256) > 0, np.bincount(outs[1].numpy().ravel(), minlength=256) > 0)
