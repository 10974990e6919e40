"""Tap-window A/B per conv and direction: the four layer4 3x3 convs of the
flagship (ResNet18, 32x32 input: 2x2 and 1x1 maps) with the clip on and off
(`set_tap_clip`), forward (conv + BN), dgrad and wgrad (one conv per flush).

Each measurement replays a captured graph of REPS calls, so the figure is
device time per call and not the host's launch rate.

Usage: python scripts/gpu_tap_clip_sweep.py [batch ...]   (default 64 1024)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from horizonml_amd import ops

CONVS = [
    # (name, in_ch, out_ch, stride, hw)
    ("layer4.0.conv1", 256, 512, 2, 2),
    ("layer4.0.conv2", 512, 512, 1, 1),   # = layer4.1.conv1 = layer4.1.conv2
    ("layer3.1.conv2", 256, 256, 1, 2),   # control: no dead tap
]
REPS = 20


def graph_us(fn, replays=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(REPS):
            fn()
    g.replay()
    torch.cuda.synchronize()
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (replays * REPS)


def main():
    C_ = ops.extension()
    batches = [int(a) for a in sys.argv[1:]] or [64, 1024]
    cl, bf = torch.channels_last, torch.bfloat16
    f32 = dict(device="cuda", dtype=torch.float32)
    was = C_.tap_clip_enabled()
    for bs in batches:
        for name, cin, cout, s, hw in CONVS:
            ho = (hw + 2 - 3) // s + 1
            x = torch.randn(bs, cin, hw, hw, device="cuda") \
                .to(memory_format=cl).to(bf)
            dz = torch.randn(bs, cout, ho, ho, device="cuda") \
                .to(memory_format=cl).to(bf)
            w = (torch.randn(cout, 3, 3, cin, device="cuda") * 0.05).to(bf)
            gam, bet = torch.ones(cout, **f32), torch.zeros(cout, **f32)
            rm, rv = torch.zeros(cout, **f32), torch.ones(cout, **f32)
            dw = torch.zeros(cout, 3, 3, cin, **f32)

            def fwd():
                C_.conv_bn_act_fwd(x, w, gam, bet, rm, rv, s, 1, 0.1, 1e-5,
                                   True, 1, None, None)

            def dgrad():
                C_.conv_dgrad_only(dz, w, hw, hw, s, 1, None, None)

            def wgrad():
                C_.wgrad_only(x, dz, cout, 3, 3, s, 1, True, dw)
                C_.flush_wgrad()

            win = tuple(C_.conv_tap_window(hw, hw, 3, 3, s, 1))
            line = f"bs={bs:<5} {name} {cin}x{hw}x{hw}->{cout} s{s} window={win}"
            for what, fn in (("fwd+bn", fwd), ("dgrad", dgrad),
                             ("wgrad", wgrad)):
                us = {}
                for on in (False, True):
                    C_.set_tap_clip(on)
                    us[on] = graph_us(fn)
                line += (f" | {what} off {us[False]:6.1f} us, "
                         f"on {us[True]:6.1f} us")
            print(line, flush=True)
    C_.set_tap_clip(was)


if __name__ == "__main__":
    main()
