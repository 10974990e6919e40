"""normalize_u8 vs augment_normalize_u8 in a replayed hipGraph chain.

Each op is captured as a chain of CHAIN dependent-stream launches and the
graph replayed; the per-call time is replay time / CHAIN, so it contains the
per-dispatch floor of a graph node as the training step sees it.  The two
ops alternate within one process (same session, same clocks) and the spread
over ROUNDS rounds is printed next to the median.

Usage: python scripts/augment_bench.py [--rounds 7] [--replays 40]
"""
import argparse
import statistics
import time

import torch

from horizonml_amd import ops as _ops

SHAPES = [(64, 3, 32, 32), (1024, 3, 32, 32), (32, 3, 224, 224)]
CHAIN = 50
MEAN = STD = 0.5


def capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(CHAIN):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def time_graph(g, replays):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(replays):
        g.replay()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / replays / CHAIN * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--replays", type=int, default=40)
    args = ap.parse_args()
    C = _ops.extension()
    dev = torch.device("cuda", 0)
    print(f"device: {torch.cuda.get_device_name(0)}  chain={CHAIN} "
          f"replays={args.replays} rounds={args.rounds}")
    print("us per call: median [min .. max] over rounds")
    for shape in SHAPES:
        g = torch.Generator().manual_seed(0)
        x = torch.randint(0, 256, shape, dtype=torch.uint8,
                          generator=g).to(dev)
        state = torch.tensor([0x5EED00001234, 0], dtype=torch.int64,
                             device=dev)
        params = torch.randint(0, 9, (shape[0],), dtype=torch.int32,
                               generator=g).to(dev) * 0x101
        graphs = {
            "normalize_u8": capture(lambda: C.normalize_u8(x, MEAN, STD)),
            "augment_normalize_u8 (rng)": capture(
                lambda: C.augment_normalize_u8(x, state, MEAN, STD, 4, True,
                                               None)),
            "augment_normalize_u8 (params)": capture(
                lambda: C.augment_normalize_u8(x, state, MEAN, STD, 4, True,
                                               params)),
        }
        times = {k: [] for k in graphs}
        for _ in range(args.rounds):  # alternate the ops within a round
            for k, gr in graphs.items():
                times[k].append(time_graph(gr, args.replays))
        nbytes = x.numel() * 3   # u8 read + bf16 write
        print(f"shape {list(shape)}  ({nbytes / 1e6:.2f} MB moved per call)")
        base = statistics.median(times["normalize_u8"])
        for k, v in times.items():
            med = statistics.median(v)
            print(f"  {k:32s} {med:8.2f} [{min(v):7.2f} .. {max(v):7.2f}]"
                  f"  x{med / base:5.2f}  {nbytes / med / 1e3:7.1f} GB/s")
        print(f"  device step counter after the run: "
              f"{int(state[1].item())}")


if __name__ == "__main__":
    main()
