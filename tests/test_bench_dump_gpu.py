"""bench.py --dump-outputs on the GPU: the rewind on the real engine
classes, and one end-to-end run of the benchmark with the option."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir)
_BENCH = os.path.join(ROOT, "bench.py")


def _load_bench():
    spec = importlib.util.spec_from_file_location("hz_bench_under_test",
                                                  _BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.gpu
@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_rewind_covers_every_buffer_a_step_updates(optimizer):
    """A step from the rewound state must equal the first step from the
    initial state BITWISE (fixed-order reductions on): any in-place updated
    buffer that state_tensors() misses — optimizer, manager, BN or extension
    state — shows up as a difference in the second step's outputs."""
    from horizonml_amd import ops as _ops
    from horizonml_amd.engine.flat import (FlatParamManager, HorizonAdam,
                                           HorizonSGD)
    from horizonml_amd.models import build_model
    from horizonml_amd.models._functional_gpu import cross_entropy
    bench = _load_bench()
    ext = _ops.extension()
    dev = torch.device("cuda", 0)
    torch.manual_seed(7)
    model = build_model("resnet18", num_classes=10).to(dev).train()
    mgr = FlatParamManager(model, dev)
    opt = (HorizonAdam(mgr, lr=1e-3) if optimizer == "adam"
           else HorizonSGD(mgr, lr=0.1))
    x = (torch.randn(8, 3, 32, 32, device=dev)
         .to(memory_format=torch.channels_last).to(torch.bfloat16))
    y = torch.randint(0, 10, (8,), device=dev)
    tensors = bench.state_tensors(mgr, opt, model)
    state0 = [t.clone() for t in tensors]

    def step():
        loss = cross_entropy(model(x), y)
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        return [loss.detach().clone(), bench.first_moment(opt).clone(),
                bench.bn_running_stats(model), mgr.master.clone(),
                mgr.shadow.clone(), mgr.rsck.clone()]

    was = ext.deterministic_enabled()
    ext.set_deterministic(True)
    try:
        first = step()
        step()  # move further away from the initial state
        bench.rewind(tensors, state0)
        again = step()
    finally:
        ext.set_deterministic(was)
        ext.set_wgrad_defer(False)
    assert float(first[1].abs().max()) > 0.0  # a gradient was computed
    for a, b in zip(first, again):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_bench_dump_outputs_end_to_end(tmp_path):
    """One tiny run of the benchmark itself: the record line, the files, and
    the timed path's forward outputs against the fixed-order recompute of
    the same step.  Bound: both run the same bf16 network from the same
    state and differ only in reduction order, which decorrelates bf16
    roundings (eps 2^-8 = 3.9e-3 per rounding); 2^-6 of the array's scale
    leaves room for a few such roundings in a row and is far below what a
    wrong kernel produces."""
    out = str(tmp_path / "dump")
    r = subprocess.run(
        [sys.executable, _BENCH, "--gpus", "1", "--steps", "3", "--warmup",
         "1", "--dump-outputs", out],
        cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec["steps"] == 3 and rec["ms_per_step"] > 0
    assert rec["config"]["exec"] == "graph"
    got = {n[:-4]: np.load(os.path.join(out, n)) for n in os.listdir(out)}
    assert sorted(got) == ["bn_running_stats", "det_bn_running_stats",
                           "det_loss", "det_opt_first_moment", "loss"]
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    for name, a in got.items():
        assert a.dtype == np.float32 and np.isfinite(a).all(), name
    assert got["loss"].shape == (1,)
    assert got["det_opt_first_moment"].size > 11e6  # ResNet18, unsampled
    assert np.abs(got["det_opt_first_moment"]).max() > 0
    for name in ("loss", "bn_running_stats"):
        fast, det = got[name], got["det_" + name]
        print(name, "max |fast - det| =", np.abs(fast - det).max(),
              "scale", np.abs(det).max())
        assert np.abs(fast - det).max() <= np.abs(det).max() * 2.0 ** -6
