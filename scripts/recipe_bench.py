"""Per-step cost of the recipe knobs on the DP flat engine (world size 1).

Runs the DP entry point on synthetic data for a few epochs per configuration
and prints epoch time / steps for every epoch after the first (the first
holds the capture warm-up tail).  Configurations alternate within one
session so clocks and neighbours are shared; the spread over epochs and
repeats is printed next to the median.

``--tree DIR`` imports the package from another checkout (to time a parent
commit with the same script); configurations that checkout does not
support are skipped.

Usage: python scripts/recipe_bench.py [--tree DIR] [--repeats 2]
           [--epochs 5] [--sample_size 25600] [--configs a,b,...]
"""
import argparse
import inspect
import os
import statistics
import sys
import tempfile

CONFIGS = {
    "adam_default": dict(optimizer_name="adam", lr=1e-3),
    "sgd_default": dict(optimizer_name="sgd", lr=0.1),
    "adam_cosine": dict(optimizer_name="adam", lr=1e-3,
                        lr_schedule="cosine", warmup_epochs=1),
    "adamw_cosine": dict(optimizer_name="adam", lr=1e-3,
                         lr_schedule="cosine", warmup_epochs=1,
                         weight_decay=1e-2, decoupled_wd=True),
    "sgd_cosine_nesterov": dict(optimizer_name="sgd", lr=0.1,
                                lr_schedule="cosine", warmup_epochs=1,
                                nesterov=True),
    "sgd_full_recipe": dict(optimizer_name="sgd", lr=0.1,
                            lr_schedule="cosine", warmup_epochs=1,
                            nesterov=True, weight_decay=5e-4,
                            label_smoothing=0.1),
    # segmented step: static table only (0 added dispatches) ...
    "sgd_nodecay": dict(optimizer_name="sgd", lr=0.1, weight_decay=5e-4,
                        no_decay_1d=True),
    # ... and with the per-step norm reduction (2 added dispatches)
    "sgd_clip": dict(optimizer_name="sgd", lr=0.1, clip_grad_norm=5.0),
    "sgd_lars_full": dict(optimizer_name="sgd", lr=0.1,
                          lr_schedule="cosine", warmup_epochs=1,
                          nesterov=True, weight_decay=5e-4,
                          label_smoothing=0.1, lars=True, clip_grad_norm=5.0,
                          no_decay_1d=True),
    "adam_clip": dict(optimizer_name="adam", lr=1e-3, clip_grad_norm=1.0),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))))
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--sample_size", type=int, default=25600)
    ap.add_argument("--batch_size", type=int, default=64)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, tree)
    os.chdir(tree)
    from data_parallel_train import run_data_parallel
    known = set(inspect.signature(run_data_parallel).parameters)
    steps = args.sample_size // args.batch_size
    print(f"tree={tree} bs={args.batch_size} "
          f"steps/epoch={steps} epochs={args.epochs} repeats={args.repeats}")
    print("ms/step (epoch_time / steps), epochs 2..: "
          "median [min .. max]  all")
    times = {}
    for rep in range(args.repeats):   # alternate the configs within a repeat
        for name in args.configs.split(","):
            kw = CONFIGS[name]
            if not set(kw) <= known:
                if rep == 0:
                    print(f"  {name:22s} skipped (not supported by this tree)")
                continue
            with tempfile.TemporaryDirectory() as d:
                df = run_data_parallel(1, args.epochs, args.sample_size, d,
                                       batch_size=args.batch_size,
                                       synthetic=True, engine="flat", **kw)
            ms = [1e3 * t / steps for t in df["epoch_time"].tolist()[1:]]
            times.setdefault(name, []).extend(ms)
    for name, v in times.items():
        print(f"  {name:22s} {statistics.median(v):7.4f} "
              f"[{min(v):7.4f} .. {max(v):7.4f}]  "
              + " ".join(f"{x:.4f}" for x in v), flush=True)


if __name__ == "__main__":
    main()
