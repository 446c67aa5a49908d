"""bench.py --dump-outputs: the arrays land as float32 / float64 .npy files, and a set larger than the cap keeps the same
leading samples of every per-sample array.  Host only."""
import os

import numpy as np
import torch

import bench


def test_dump_writes_every_output_as_float(tmp_path):
    B = 16
    lp, grad = torch.randn(B), torch.randn(B, 5, dtype=torch.float64)
    bench.dump_outputs(str(tmp_path), (("log_prob", lp, True), ("grad_z", grad, True), ("buf", torch.arange(7), False)), B)
    assert sorted(os.listdir(tmp_path)) == ["buf.npy", "grad_z.npy", "log_prob.npy"]
    assert np.array_equal(np.load(tmp_path / "log_prob.npy"), lp.numpy())
    assert np.load(tmp_path / "grad_z.npy").dtype == np.float64
    assert np.array_equal(np.load(tmp_path / "buf.npy"), np.arange(7, dtype=np.float32))


def test_dump_keeps_leading_samples_under_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 1000)
    B = 64
    lp, grad = torch.randn(B), torch.randn(B, 3)
    bench.dump_outputs(str(tmp_path), (("log_prob", lp, True), ("grad_z", grad, True), ("buf", torch.ones(10), False)), B)
    kept = np.load(tmp_path / "log_prob.npy")
    assert len(kept) == (1000 - 40) // 16
    assert np.array_equal(kept, lp[:len(kept)].numpy())
    assert np.array_equal(np.load(tmp_path / "grad_z.npy"), grad[:len(kept)].numpy())
    assert np.load(tmp_path / "buf.npy").shape == (10,)
