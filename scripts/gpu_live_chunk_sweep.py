"""Chunk-size sweep of the live-range optimizer step (docs/TUNING.md,
``LIVE_CHUNK``) at ResNet18@32's real live table.

Usage: python scripts/gpu_live_chunk_sweep.py

One backward fills the tap-window registry; the table is then rebuilt per
chunk size and ``adam_step_live`` / ``sgd_step_live`` are timed against the
full-range ops: a graph of 40 steps, replayed, time per step from device
events, once with the state left in the Infinity Cache and once with a 512 MB
fill in front of every step.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from horizonml_amd import ops as _ops
from horizonml_amd.engine.flat import (FlatParamManager, HorizonAdam,
                                       build_live_chunks)
from horizonml_amd.models import resnet18
from horizonml_amd.models._functional_gpu import cross_entropy

ext = _ops.extension()
dev = torch.device("cuda", 0)
torch.manual_seed(0)
model = resnet18(num_classes=10).to(dev)
mgr = FlatParamManager(model, dev)
opt = HorizonAdam(mgr, lr=1e-3)
x = torch.randn(8, 3, 32, 32, device=dev).to(
    memory_format=torch.channels_last).to(torch.bfloat16)
y = torch.randint(0, 10, (8,), device=dev)
cross_entropy(model(x), y).backward()
ext.flush_wgrad()
torch.cuda.synchronize()
wins = [w for w in mgr.live_windows() if w[6] * w[8] < w[2] * w[3]]
print("clipped windows:", wins, flush=True)
n = mgr.numel
mom = torch.zeros_like(mgr.master)


def timeit(fn, inner=40, reps=10):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(inner):
            fn()
    g.replay()
    torch.cuda.synchronize()
    best = []
    for _ in range(reps):
        a, b = torch.cuda.Event(True), torch.cuda.Event(True)
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize()
        best.append(a.elapsed_time(b) * 1000 / inner)
    best.sort()
    return best[0], best[len(best) // 2]


def adam_full():
    ext.adam_step(mgr.master, mgr.grad, opt.m, opt.v, mgr.shadow, opt.step_t,
                  1e-3, 0.9, 0.999, 1e-8, 0.0, True, mgr.stats_arena, None,
                  1.0, None, None, None)


def sgd_full():
    ext.sgd_step(mgr.master, mgr.grad, mom, mgr.shadow, 0.1, 0.9, 0.0, True,
                 None, 1.0, None, None, None)


# something else between steps so the state is not simply cache-resident:
# a 512 MB fill evicts the 256 MB Infinity Cache
evict = torch.empty(128 << 20, device=dev)


def with_evict(fn):
    def f():
        evict.fill_(1.0)
        fn()
    return f


def fill_only():
    evict.fill_(1.0)


print("us/step (min, median); 'cold' = 512 MB fill in front of every step, "
      "fill time subtracted", flush=True)
f0 = timeit(fill_only)
print(f"fill alone {f0[0]:.1f} {f0[1]:.1f}")
for name, full in (("adam", adam_full), ("sgd", sgd_full)):
    t = timeit(full)
    c = timeit(with_evict(full))
    print(f"{name} full-range: warm {t[0]:.1f} {t[1]:.1f}  cold "
          f"{c[0] - f0[0]:.1f} {c[1] - f0[1]:.1f}", flush=True)
    for chunk in (1024, 2048, 4096, 8192, 16384):
        chunks, n_dead = build_live_chunks(n, wins, chunk)
        tab = torch.tensor(chunks, dtype=torch.int32, device=dev)
        if name == "adam":
            def live():
                ext.adam_step_live(mgr.master, mgr.grad, opt.m, opt.v,
                                   mgr.shadow, opt.step_t, None, None, 1e-3,
                                   0.9, 0.999, 1e-8, True, tab,
                                   mgr.stats_arena, None, 1.0, None, None,
                                   None)
        else:
            def live():
                ext.sgd_step_live(mgr.master, mgr.grad, mom, mgr.shadow,
                                  None, None, None, 0.1, 0.9, False, True,
                                  tab, None, 1.0, None, None, None)
        t = timeit(live)
        c = timeit(with_evict(live))
        print(f"{name} live chunk={chunk:6d} nchunks={len(chunks):5d} "
              f"dead={n_dead}: warm {t[0]:.1f} {t[1]:.1f}  cold "
              f"{c[0] - f0[0]:.1f} {c[1] - f0[1]:.1f}", flush=True)
