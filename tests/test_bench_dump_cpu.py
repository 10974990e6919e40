"""bench.py --dump-outputs helpers, on CPU tensors: file names, dtype, the
64 MB ceiling, and that the sample of an over-budget array is the same from
call to call (two builds must be comparable array for array).  The end to
end run and the rewind on the real engine classes are in
test_bench_dump_gpu.py."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

_BENCH = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir,
                      "bench.py")


def _load_bench():
    spec = importlib.util.spec_from_file_location("hz_bench_under_test",
                                                  _BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _model():
    torch.manual_seed(0)
    m = nn.Sequential(nn.Conv2d(3, 4, 3), nn.BatchNorm2d(4),
                      nn.Conv2d(4, 6, 3), nn.BatchNorm2d(6))
    m[1].running_mean.copy_(torch.arange(4.0))
    m[3].running_var.copy_(torch.arange(6.0) + 2.0)
    return m


def test_write_arrays(tmp_path):
    bench = _load_bench()
    model = _model()
    grad = torch.arange(1000.0).reshape(10, 100) * 0.5
    out = str(tmp_path / "dump")
    bench.write_arrays(out, {
        "loss": torch.tensor(2.25, dtype=torch.bfloat16),
        "bn_running_stats": bench.bn_running_stats(model),
        "det_opt_first_moment": grad})
    assert sorted(os.listdir(out)) == ["bn_running_stats.npy",
                                       "det_opt_first_moment.npy",
                                       "loss.npy"]
    got = {n[:-4]: np.load(os.path.join(out, n)) for n in os.listdir(out)}
    assert all(a.dtype == np.float32 for a in got.values())
    assert got["loss"].tolist() == [2.25]
    np.testing.assert_array_equal(got["det_opt_first_moment"],
                                  grad.flatten().numpy())
    # running mean/var of every BN, module order
    want = torch.cat([model[1].running_mean, model[1].running_var,
                      model[3].running_mean, model[3].running_var])
    np.testing.assert_array_equal(got["bn_running_stats"], want.numpy())


def test_write_arrays_sample_is_fixed_and_bounded(tmp_path, monkeypatch):
    bench = _load_bench()
    assert bench.DUMP_ARRAY_BUDGET_BYTES < (64 << 20)
    # shrink the budget instead of allocating a >48 MB buffer in a test
    monkeypatch.setattr(bench, "DUMP_ARRAY_BUDGET_BYTES", 4 * 100)
    runs = []
    for name in ("a", "b"):
        out = str(tmp_path / name)
        bench.write_arrays(out, {"g": torch.arange(1000.0),
                                 "small": torch.arange(100.0)})
        runs.append(np.load(os.path.join(out, "g.npy")))
        np.testing.assert_array_equal(
            np.load(os.path.join(out, "small.npy")), np.arange(100.0))
    assert runs[0].shape == (100,)
    np.testing.assert_array_equal(runs[0], runs[1])
    # a sample of the buffer itself, in buffer order, without repeats
    assert np.all(np.diff(runs[0]) > 0)
    assert set(runs[0].tolist()) <= set(range(1000))


def test_rewind_restores_in_place():
    bench = _load_bench()
    ts = [torch.arange(4.0), torch.ones(2, 2)]
    ptrs = [t.data_ptr() for t in ts]
    snap = [t.clone() for t in ts]
    ts[0].mul_(3.0)
    ts[1].zero_()
    bench.rewind(ts, snap)
    assert [t.data_ptr() for t in ts] == ptrs  # graph-captured addresses
    for t, s in zip(ts, snap):
        assert torch.equal(t, s)


def test_first_moment_picks_the_gradient_buffer():
    bench = _load_bench()

    class _Adam:
        m = torch.ones(3)

    class _SGD:
        mom = torch.zeros(3)

    class _SGDNoMomentum:
        mom = None

    assert bench.first_moment(_Adam()) is _Adam.m
    assert bench.first_moment(_SGD()) is _SGD.mom
    with pytest.raises(ValueError):
        bench.first_moment(_SGDNoMomentum())


def test_cli_has_dump_outputs_and_full(monkeypatch):
    bench = _load_bench()
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps",
                                     "7", "--warmup", "2"])
    a = bench.parse_args()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr("sys.argv", ["bench.py", "--full", "--dump-outputs",
                                     "d"])
    a = bench.parse_args()
    assert a.full is True and a.dump_outputs == "d"
