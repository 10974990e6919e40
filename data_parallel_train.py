#!/usr/bin/env python3
"""Data-parallel training entrypoint (strategy 1).

CLI/CSV parity with the reference's ``data_parallel_train.py`` (flags
``--world_size --epochs --sample_size``, per-worker CSVs + combined CSV in
``data_parallel_logs/``), rebuilt on the MI355X-native engine:
one process per GPU, bf16 bucketed RCCL all-reduce over xGMI, gfx950 HIP
kernels for the ResNet hot path.  On CPU-only hosts it runs the gloo
plumbing configuration (BASELINE.json config #1).
"""
from __future__ import annotations

import argparse

from horizonml_amd.engine.dp import dp_worker
from horizonml_amd.runtime.launcher import run_workers


def run_data_parallel(world_size: int, epochs: int, sample_size: int,
                      logs_dir: str = "data_parallel_logs",
                      batch_size: int = 64, model_name: str = "resnet18",
                      backend=None, synthetic=None, lr: float = 1e-3,
                      optimizer_name: str = "adam", engine: str = "auto",
                      checkpoint_path=None, per_step_barrier: bool = False,
                      augment: bool = False, augment_pad: int = 4,
                      lr_schedule: str = "constant",
                      warmup_epochs: float = 0.0, min_lr: float = 0.0,
                      lr_milestones=(), lr_gamma: float = 0.1,
                      weight_decay: float = 0.0, nesterov: bool = False,
                      decoupled_wd: bool = False,
                      label_smoothing: float = 0.0,
                      no_decay_1d: bool = False, clip_grad_norm: float = 0.0,
                      lars: bool = False, lars_eta: float = 1e-3):
    """Launcher parity with reference ``run_data_parallel``
    (``data_parallel_train.py:233-291``). Returns the combined DataFrame.

    ``augment`` (an extension over the reference): random crop with
    ``augment_pad`` zero padding + horizontal flip, fused into the on-device
    normalize.  ``lr_schedule`` … ``label_smoothing`` (extensions too): the
    training-recipe knobs of ``engine.dp.train_dp_flat``; epoch quantities
    are converted to steps with the rank's loader length.  ``no_decay_1d``
    (no weight decay on BN and bias parameters), ``clip_grad_norm`` (global
    L2 norm, 0 = off), ``lars`` / ``lars_eta`` (SGD only) likewise."""
    if lars and optimizer_name.lower() == "adam":
        raise ValueError("lars needs optimizer_name='sgd'")
    return run_workers(dp_worker, world_size, epochs, sample_size, logs_dir,
                       timeout_base=120,
                       extra_args=(batch_size, model_name, backend, synthetic,
                                   lr, optimizer_name, engine,
                                   checkpoint_path, per_step_barrier,
                                   augment, augment_pad, lr_schedule,
                                   warmup_epochs, min_lr,
                                   tuple(lr_milestones), lr_gamma,
                                   weight_decay, nesterov, decoupled_wd,
                                   label_smoothing, no_decay_1d,
                                   clip_grad_norm, lars, lars_eta))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Data-parallel training")
    ap.add_argument("--world_size", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--sample_size", type=int, default=1000)
    ap.add_argument("--logs_dir", type=str, default="data_parallel_logs")
    ap.add_argument("--batch_size", type=int, default=64)
    ap.add_argument("--model", type=str, default="resnet18")
    ap.add_argument("--backend", type=str, default=None,
                    choices=[None, "nccl", "gloo"], nargs="?")
    ap.add_argument("--synthetic", action="store_true", default=None,
                    help="force synthetic CIFAR-shaped data")
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--deterministic", action="store_true",
                    help="torch.use_deterministic_algorithms (GPU kernels "
                         "remain reproducible only to bf16/atomic rounding)")
    ap.add_argument("--optimizer", type=str, default="adam",
                    choices=["adam", "sgd"])
    ap.add_argument("--engine", type=str, default="auto",
                    choices=["auto", "eager", "flat"],
                    help="flat = hipGraph/fused fast path (GPU default); "
                         "eager = bucketed-DDP torch-optimizer loop")
    ap.add_argument("--checkpoint", type=str, default=None,
                    help="checkpoint file: saved per epoch (rank 0), "
                         "resumed from when it exists")
    ap.add_argument("--per_step_barrier", action="store_true",
                    help="restore the reference's full-world barrier after "
                         "every step (exact idle_time semantics; the "
                         "default barriers per epoch)")
    ap.add_argument("--augment", action="store_true",
                    help="RandomCrop(32, padding=augment_pad) + "
                         "RandomHorizontalFlip, fused into the on-device "
                         "normalize kernel (default off)")
    ap.add_argument("--augment_pad", type=int, default=4,
                    help="zero padding of the random crop (with --augment)")
    ap.add_argument("--lr_schedule", type=str, default="constant",
                    choices=["constant", "cosine", "linear", "multistep"],
                    help="learning-rate schedule over the whole run; the "
                         "flat engine reads it on the device, inside the "
                         "captured step (default constant = --lr)")
    ap.add_argument("--warmup_epochs", type=float, default=0.0,
                    help="linear warm-up to --lr over this many epochs")
    ap.add_argument("--min_lr", type=float, default=0.0,
                    help="final lr of the cosine / linear schedules")
    ap.add_argument("--lr_milestones", type=int, nargs="*", default=[],
                    help="epochs at which multistep multiplies the lr by "
                         "--lr_gamma")
    ap.add_argument("--lr_gamma", type=float, default=0.1)
    ap.add_argument("--weight_decay", type=float, default=0.0,
                    help="L2 weight decay on every parameter (BN and bias "
                         "included, unless --no_decay_1d)")
    ap.add_argument("--nesterov", action="store_true",
                    help="Nesterov momentum (with --optimizer sgd)")
    ap.add_argument("--decoupled_wd", action="store_true",
                    help="AdamW: decoupled weight decay (with --optimizer "
                         "adam)")
    ap.add_argument("--label_smoothing", type=float, default=0.0)
    ap.add_argument("--no_decay_1d", action="store_true",
                    help="no weight decay on 1-D parameters (BN weight/bias, "
                         "biases)")
    ap.add_argument("--clip_grad_norm", type=float, default=0.0,
                    help="clip the gradient to this global L2 norm "
                         "(0 = off)")
    ap.add_argument("--lars", action="store_true",
                    help="LARS layer-wise trust ratio (with --optimizer sgd)")
    ap.add_argument("--lars_eta", type=float, default=1e-3,
                    help="LARS trust coefficient")
    args = ap.parse_args(argv)
    if args.lars and args.optimizer == "adam":
        ap.error("--lars needs --optimizer sgd")
    if args.clip_grad_norm < 0 or args.lars_eta <= 0:
        ap.error("--clip_grad_norm must be >= 0 and --lars_eta > 0")
    return args


def main(argv=None):
    args = parse_args(argv)
    if args.deterministic:
        import os
        os.environ["HZ_DETERMINISTIC"] = "1"
    df = run_data_parallel(args.world_size, args.epochs, args.sample_size,
                           args.logs_dir, args.batch_size, args.model,
                           args.backend, args.synthetic, args.lr,
                           args.optimizer, args.engine, args.checkpoint,
                           args.per_step_barrier, args.augment,
                           args.augment_pad, args.lr_schedule,
                           args.warmup_epochs, args.min_lr,
                           args.lr_milestones, args.lr_gamma,
                           args.weight_decay, args.nesterov,
                           args.decoupled_wd, args.label_smoothing,
                           args.no_decay_1d, args.clip_grad_norm, args.lars,
                           args.lars_eta)
    if df is not None:
        print(df.tail(args.world_size).to_string(index=False))


if __name__ == "__main__":
    main()
