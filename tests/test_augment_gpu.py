"""GPU side of the fused random crop + flip + normalize kernel
(``k_augment_normalize_u8``): bitwise agreement with ``k_normalize_u8`` on
the Python-built reference, device-side counter under eager calls and graph
replay, argument checks, and the ``--augment`` flag on both DP engines."""
import numpy as np
import pytest
import torch

from horizonml_amd.data.augment import (DeviceAugment, augment_params,
                                        augment_reference, pack_params)

pytestmark = pytest.mark.gpu

MEAN = STD = 0.5
KEY = (0x5EED1234 << 32) | 0x9ABCDEF1   # bits above 32 set


@pytest.fixture(scope="module")
def ext():
    from horizonml_amd import ops as _ops
    return _ops.extension()


def _dev():
    return torch.device("cuda", 0)


def _batch(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, shape, dtype=torch.uint8,
                         generator=g).to(_dev())


def _state(key, step):
    skey = key - (1 << 64) if key >= (1 << 63) else key
    return torch.tensor([skey, step], dtype=torch.int64, device=_dev())


def _expected(ext, x, dy, dx, fl, pad):
    return ext.normalize_u8(augment_reference(x, dy, dx, fl, pad)
                            .contiguous(), MEAN, STD)


def _check_out(y, ref):
    assert y.dtype == torch.bfloat16 and y.shape == ref.shape
    assert y.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(y, ref)


@pytest.mark.parametrize("shape,pad", [((5, 3, 32, 32), 4),
                                       ((3, 3, 17, 9), 2),
                                       ((2, 1, 8, 8), 3),
                                       ((2, 4, 6, 5), 1)])
def test_explicit_params_bitwise(ext, shape, pad):
    x = _batch(shape, 1)
    p = pad
    cases = [(0, 0, 0), (2 * p, 2 * p, 1), (0, 2 * p, 1), (2 * p, 0, 0),
             (p, p, 1)]
    # every case on every sample position (5 launches of one tiny kernel)
    for rot in range(len(cases)):
        cyc = [cases[(n + rot) % len(cases)] for n in range(shape[0])]
        dy, dx, fl = (torch.tensor(c) for c in zip(*cyc))
        state = _state(KEY, 11)
        y = ext.augment_normalize_u8(x, state, MEAN, STD, pad, True,
                                     pack_params(dy, dx, fl).to(_dev()))
        _check_out(y, _expected(ext, x, dy, dx, fl, pad))
        assert state.tolist()[1] == 11   # counter untouched


@pytest.mark.parametrize("shape", [(4, 3, 32, 32), (1, 3, 224, 224)])
def test_identity_rng_mode(ext, shape):
    x = _batch(shape, 2)
    state = _state(KEY, 5)
    y = ext.augment_normalize_u8(x, state, MEAN, STD, 0, False, None)
    _check_out(y, ext.normalize_u8(x, MEAN, STD))
    assert state.tolist()[1] == 6


@pytest.mark.parametrize("shape,pad", [((70, 3, 32, 32), 4),
                                       ((9, 3, 17, 9), 2)])
def test_rng_mode_matches_python_hash(ext, shape, pad):
    x = _batch(shape, 3)
    step0 = 2 ** 32 - 1   # the second call wraps the low word
    state = _state(KEY, step0)
    for k in range(2):
        y = ext.augment_normalize_u8(x, state, MEAN, STD, pad, True, None)
        dy, dx, fl = augment_params(KEY, step0 + k, shape[0], pad)
        _check_out(y, _expected(ext, x, dy, dx, fl, pad))
    assert state.tolist()[1] == step0 + 2   # advanced by exactly 2
    skey = KEY - (1 << 64) if KEY >= (1 << 63) else KEY
    assert state[0].item() == skey


def test_graph_replay_advances_counter(ext):
    x = _batch((64, 3, 32, 32), 4)
    aug = DeviceAugment(KEY, pad=4, flip=True, device=_dev())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        aug(x)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    aug.set_step(7)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y = aug(x)
    assert aug.step() == 7   # capture launched nothing
    outs = []
    for _ in range(3):
        g.replay()
        outs.append(y.clone())
    torch.cuda.synchronize()
    for k, out in enumerate(outs):
        dy, dx, fl = augment_params(KEY, 7 + k, 64, 4)
        assert torch.equal(out, _expected(ext, x, dy, dx, fl, 4))
    assert not torch.equal(outs[0], outs[1])
    assert not torch.equal(outs[1], outs[2])
    assert not torch.equal(outs[0], outs[2])
    assert aug.step() == 10


def test_argument_checks(ext):
    x = _batch((2, 3, 8, 8), 5)
    state = _state(KEY, 0)

    def call(x_=x, state_=state, pad=2, params=None):
        return ext.augment_normalize_u8(x_, state_, MEAN, STD, pad, True,
                                        params)

    with pytest.raises(RuntimeError):
        call(pad=128)
    with pytest.raises(RuntimeError):
        call(state_=state.cpu())
    with pytest.raises(RuntimeError):
        call(state_=state.to(torch.int32))
    with pytest.raises(RuntimeError):
        call(params=torch.zeros(3, dtype=torch.int32, device=_dev()))
    with pytest.raises(RuntimeError):
        call(x_=_batch((2, 8, 8, 3), 5).permute(0, 3, 1, 2))
    torch.cuda.synchronize()
    assert state.tolist()[1] == 0   # nothing was launched
    call()                                 # the valid call still works
    assert state.tolist()[1] == 1


_COLS = ["epoch", "loss", "accuracy", "epoch_time", "avg_step_time",
         "compute_time", "comm_time", "idle_time", "avg_cpu", "avg_memory",
         "grad_divergence", "worker", "total_training_time"]


def _run(tmp_path, tag, engine, augment):
    from data_parallel_train import run_data_parallel
    df = run_data_parallel(1, 2, 128, str(tmp_path / tag), batch_size=32,
                           synthetic=True, engine=engine, augment=augment)
    assert df is not None and len(df) == 2
    assert set(_COLS).issubset(df.columns)
    assert np.isfinite(df["loss"].to_numpy()).all()
    return float(df[df["epoch"] == 1]["loss"].iloc[0])


@pytest.mark.timeout(300)
def test_dp_eager_augment_gpu(tmp_path):
    _run(tmp_path, "eager", "eager", True)


@pytest.mark.timeout(300)
def test_dp_flat_augment_gpu(tmp_path, monkeypatch):
    monkeypatch.setenv("HZ_DETERMINISTIC", "1")
    a = _run(tmp_path, "a", "flat", True)
    b = _run(tmp_path, "b", "flat", True)
    off = _run(tmp_path, "off", "flat", False)
    assert a == b, (a, b)
    assert a != off, (a, off)
