"""Wide classifier head: linear forward, linear backward and cross-entropy
with the wide kernels on and off (HZ_LINEAR_WIDE / HZ_CE_WIDE), same process.

Each (shape, op, state) is a captured graph of CHAIN back-to-back calls,
replayed REPLAYS times per sample between device events; the two states
alternate, SAMPLES samples each.  Reported: median [min .. max] µs per call,
and the largest |on − off| of the outputs.  Off is the former code path.

Usage: python scripts/gpu_head_wide_bench.py > profiles/<name>.txt
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from horizonml_amd import ops

SHAPES = [(32, 2048, 1000), (256, 2048, 1000), (64, 512, 100),
          (1024, 512, 100)]
CHAIN, REPLAYS, SAMPLES = 20, 10, 5


def capture(fn):
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(3):
            out = fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(CHAIN):
            out = fn()
    return g, out


def sample(g):
    a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    a.record()
    for _ in range(REPLAYS):
        g.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / (REPLAYS * CHAIN)


def main():
    C = ops.extension()
    assert torch.cuda.is_available(), "needs a GPU"
    print(f"chain={CHAIN} replays={REPLAYS} samples={SAMPLES}; µs per call, "
          "median [min .. max]")
    for B, In, Out in SHAPES:
        g = torch.Generator().manual_seed(B + In + Out)
        x = torch.randn(B, In, generator=g).bfloat16().cuda()
        w = (torch.randn(Out, In, generator=g) * 0.05).bfloat16().cuda()
        b = torch.randn(Out, generator=g).cuda()
        dy = (torch.randn(B, Out, generator=g) / B).cuda()
        logits = torch.randn(B, Out, generator=g).cuda()
        tgt = torch.randint(0, Out, (B,), generator=g).cuda()
        opsets = {
            "linear_fwd": lambda: (C.linear_fwd(x, w, b),),
            "linear_bwd": lambda: C.linear_bwd(dy, x, w, True, True, None,
                                               None),
            "ce": lambda: C.cross_entropy_fwd_bwd(logits, tgt),
        }
        for name, fn in opsets.items():
            graphs, outs = {}, {}
            for on in (True, False):
                C.set_linear_wide(on)
                C.set_ce_wide(on)
                graphs[on], outs[on] = capture(fn)
            for gr in graphs.values():
                gr.replay()
            torch.cuda.synchronize()
            t = {True: [], False: []}
            for _ in range(SAMPLES):
                for on in (True, False):
                    t[on].append(sample(graphs[on]))
            diff = max(float((p.float() - q.float()).abs().max())
                       for p, q in zip(outs[True], outs[False]))
            fmt = {on: f"{statistics.median(v):9.2f} [{min(v):9.2f} .. "
                       f"{max(v):9.2f}]" for on, v in t.items()}
            print(f"[{B:5d},{In:5d},{Out:5d}] {name:10s} on {fmt[True]}  "
                  f"off {fmt[False]}  off/on "
                  f"{statistics.median(t[False]) / statistics.median(t[True]):6.2f}"
                  f"  max|on-off| {diff:.3e}")
    C.set_linear_wide(True)
    C.set_ce_wide(True)


if __name__ == "__main__":
    main()
