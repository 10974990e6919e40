"""Channel-owner BN kernels vs the two-kernel pairs they replace, in
isolation, at the flagship's (ResNet18 / CIFAR / batch 64) shapes.

Each variant is captured as a chain of REPS dependent launches in one
hipGraph and replayed, so the figure is device time per pair INCLUDING the
launch boundaries it pays inside a captured training step (two for the
pair, one for the owner kernel).  lpr = lanes per row of the owner kernel
(4*lpr channels per workgroup); "pair" is the existing reduce + apply.

Usage: python scripts/gpu_bn_owner_sweep.py   (sets the defaults and M
limits documented in docs/TUNING.md)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from horizonml_amd import ops

REPS = 40
ROUNDS = 25

# (M, C, nsplit) of the split-K forward convs: layer2, layer3, layer4, and
# one shape class up (batch 256) to place the M limit
FWD = [(1024, 128, 8), (256, 256, 16), (64, 512, 32),
       (512, 256, 8), (2048, 128, 8), (3840, 128, 4), (1024, 256, 8)]
# (M, C, mask) of the same-call backward BN: conv2 of every block (mask 1)
# and the 1x1 downsample convs (mask 0); then the classes between the
# flagship's and layer4 at batch 1024 that place the M*C limit, and the
# larger-M classes for the M limit
BWD = [(4096, 64, 1), (1024, 128, 1), (256, 256, 1), (64, 512, 1),
       (1024, 128, 0), (256, 256, 0), (64, 512, 0),
       (1024, 136, 1), (1024, 256, 1), (512, 512, 1), (1024, 512, 1),
       (1024, 512, 0),
       (2048, 128, 1), (4096, 64, 2), (8192, 64, 1), (16384, 64, 2),
       (4096, 256, 1)]


def time_chain(fn):
    """us per call of fn inside a replayed graph of REPS dependent calls."""
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(REPS):
                fn()
    torch.cuda.synchronize()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    best, tot = 1e9, 0.0
    for _ in range(ROUNDS):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        t = e0.elapsed_time(e1) * 1e3 / REPS
        best = min(best, t)
        tot += t
    return tot / ROUNDS, best


def main():
    C_ = ops.extension()
    C_.set_bn_owner(True)
    dev = "cuda"
    print(f"REPS={REPS} ROUNDS={ROUNDS}; us per pair, mean (min)")
    print("-- forward: k_stats_reduce + k_bn_apply_v8<F32SRC>  vs  "
          "k_bn_fwd_owner")
    for M, C, ns in FWD:
        ws = torch.randn(ns, M, C, device=dev)
        res = torch.randn(M, C, device=dev).bfloat16()
        y = torch.empty(M, C, device=dev, dtype=torch.bfloat16)
        co = torch.empty_like(y)
        stats = torch.zeros(2 * C, device=dev)
        g, b = torch.ones(C, device=dev), torch.zeros(C, device=dev)
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        sm, si = torch.empty(C, device=dev), torch.empty(C, device=dev)
        row = f"M={M:>6} C={C:>4} nsplit={ns:>2}:"
        for lpr in (0, 1, 2, 4, 8):
            if lpr and M * lpr * 16 > 60 * 1024:
                row += f"  lpr{lpr}      n/a     "
                continue
            mean, best = time_chain(lambda: C_.bn_fwd_pair_bench(
                ws, res, y, co, stats, g, b, rm, rv, sm, si, M, C, ns, 1,
                lpr))
            row += f"  {'pair' if lpr == 0 else 'lpr%d' % lpr} " \
                   f"{mean:6.2f} ({best:6.2f})"
        print(row, flush=True)
    print("-- backward: k_bnact_bwd_reduce + k_bn_bwd_apply_v8  vs  "
          "k_bn_bwd_owner")
    for M, C, mask in BWD:
        dy = torch.randn(M, C, device=dev).bfloat16()
        yy = torch.randn(M, C, device=dev).bfloat16()
        x = torch.randn(M, C, device=dev).bfloat16()
        mean_ = torch.randn(C, device=dev)
        istd = torch.rand(C, device=dev) + 0.5
        g, b = torch.randn(C, device=dev), torch.randn(C, device=dev)
        sdz, sdzx = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        dconv = torch.empty_like(dy)
        dres = torch.empty_like(dy) if mask in (1, 3) else None
        row = f"M={M:>6} C={C:>4} mask={mask}:    "
        for lpr in (0, 1, 2, 4, 8):
            mean, best = time_chain(lambda: C_.bn_bwd_pair_bench(
                dy, yy, x, mean_, istd, g, b, sdz, sdzx, dconv, dres, M, C,
                mask, lpr))
            row += f"  {'pair' if lpr == 0 else 'lpr%d' % lpr} " \
                   f"{mean:6.2f} ({best:6.2f})"
        print(row, flush=True)


if __name__ == "__main__":
    main()
