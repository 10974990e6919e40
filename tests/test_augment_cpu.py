"""CPU side of the fused random crop + flip + normalize feature: the hash
mirror (``augment_params``), the gather mirror (``augment_reference``), the
``DeviceAugment`` CPU path and the ``--augment`` flag on the gloo engine."""
import pytest
import torch

from horizonml_amd.data import (DeviceAugment, augment_params,
                                augment_reference)
from horizonml_amd.data.cifar import normalize_uint8

KEY = (1234 << 32) | 5   # fixed; checked below for coverage at step 3
STEP = 3


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _coincide(a, b):
    """Fraction of samples whose whole (dy, dx, fl) triple coincides."""
    eq = (a[0] == b[0]) & (a[1] == b[1]) & (a[2] == b[2])
    return eq.float().mean().item()


def test_augment_params_deterministic():
    a = augment_params(KEY, STEP, 256, 4)
    assert _same(a, augment_params(KEY, STEP, 256, 4))
    for t in a:
        assert t.dtype == torch.int64 and t.shape == (256,)
    # another step / key: fewer than a quarter of the samples coincide
    assert _coincide(a, augment_params(KEY, STEP + 1, 256, 4)) < 0.25
    assert _coincide(a, augment_params(KEY + 1, STEP, 256, 4)) < 0.25
    assert _coincide(a, augment_params(KEY ^ (1 << 40), STEP, 256, 4)) < 0.25
    # another sample index: the stream shifted by one sample
    b = augment_params(KEY, STEP, 257, 4)
    assert _coincide(a, tuple(t[1:] for t in b)) < 0.25
    # only the low 32 bits of the step enter the hash
    assert _same(a, augment_params(KEY, STEP + (1 << 32), 256, 4))


def test_augment_params_range_and_coverage():
    dy, dx, fl = augment_params(KEY, STEP, 8192, 4)
    assert dy.min() >= 0 and dy.max() <= 8
    assert dx.min() >= 0 and dx.max() <= 8
    assert set(fl.tolist()) == {0, 1}
    cells = set(zip(dy.tolist(), dx.tolist(), fl.tolist()))
    assert len(cells) == 9 * 9 * 2
    frac = fl.float().mean().item()
    assert 0.47 <= frac <= 0.53, frac
    _, _, fl0 = augment_params(KEY, STEP, 8192, 4, flip=False)
    assert not fl0.any()
    dy0, dx0, _ = augment_params(KEY, STEP, 8192, 0)
    assert not dy0.any() and not dx0.any()


def test_augment_reference_hand_built():
    x = torch.arange(1, 13, dtype=torch.uint8).view(1, 1, 3, 4)

    def run(dy, dx, fl):
        out = augment_reference(x, torch.tensor([dy]), torch.tensor([dx]),
                                torch.tensor([fl]), 1)
        assert out.dtype == torch.uint8 and out.shape == x.shape
        return out[0, 0].tolist()

    assert run(0, 0, 0) == [[0, 0, 0, 0], [0, 1, 2, 3], [0, 5, 6, 7]]
    assert run(2, 2, 0) == [[6, 7, 8, 0], [10, 11, 12, 0], [0, 0, 0, 0]]
    assert run(1, 1, 1) == [[4, 3, 2, 1], [8, 7, 6, 5], [12, 11, 10, 9]]
    # flip AFTER crop: the window's zero column lands on the right (flipping
    # the image first would give [0, 4, 3, 2] rows)
    assert run(0, 0, 1) == [[0, 0, 0, 0], [3, 2, 1, 0], [7, 6, 5, 0]]


def test_device_augment_cpu():
    g = torch.Generator().manual_seed(0)
    xs = [torch.randint(0, 256, (6, 3, 8, 8), dtype=torch.uint8, generator=g)
          for _ in range(3)]
    a, b = DeviceAugment(KEY, pad=2), DeviceAugment(KEY, pad=2)
    outs = []
    for k, x in enumerate(xs):
        ya, yb = a(x), b(x)
        assert ya.dtype == torch.float32 and ya.shape == x.shape
        assert torch.equal(ya, yb)
        dy, dx, fl = augment_params(KEY, k, 6, 2)
        assert torch.equal(
            ya, normalize_uint8(augment_reference(x, dy, dx, fl, 2)))
        outs.append(ya)
    assert a.step() == 3
    c = DeviceAugment(KEY, pad=2)
    c.set_step(1)
    assert torch.equal(c(xs[1]), outs[1])
    with pytest.raises(ValueError):
        DeviceAugment(KEY, pad=128)


@pytest.mark.timeout(300)
def test_dp_gloo_augment_flag(tmp_path):
    import pandas as pd

    from data_parallel_train import run_data_parallel
    losses = {}
    for aug in (True, False):
        logs = str(tmp_path / f"aug{int(aug)}")
        df = run_data_parallel(1, 2, 64, logs, backend="gloo",
                               synthetic=True, engine="eager", batch_size=32,
                               augment=aug)
        assert df is not None and len(df) == 2
        assert set(["epoch", "loss", "accuracy", "epoch_time",
                    "avg_step_time", "compute_time", "comm_time",
                    "idle_time", "avg_cpu", "avg_memory", "grad_divergence",
                    "worker", "total_training_time"]).issubset(df.columns)
        w = pd.read_csv(f"{logs}/worker_0_samples_64.csv")
        assert list(w["epoch"]) == [1, 2]
        assert w["loss"].notna().all()
        losses[aug] = float(w["loss"].iloc[0])
    assert losses[True] != losses[False]
