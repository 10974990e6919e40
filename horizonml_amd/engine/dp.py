"""Data-parallel training engine (strategy 1).

MI355X-native rebuild of the reference DP loop
(``data_parallel_train.py:76-230``): per-epoch barrier + per-step metrics +
CSV flush per epoch, but with

* our ``BucketedDataParallel`` (bf16 bucketed RCCL all-reduce overlapping
  backward) instead of torch DDP over gloo,
* honest compute/comm/idle segmentation on hipEvents (Q4 fix),
* bf16 channels-last execution through the gfx950 kernels on GPU.

The per-step full-world barrier of the reference
(``data_parallel_train.py:150-152``) serializes every step; we keep the
semantics (idle accounting of peer skew) per epoch, not per step, and
document the deviation — per-step barriers on an 8-GPU RCCL ring would
dominate the microsecond-scale steps.
"""
from __future__ import annotations

import os
import time
from typing import Optional

import torch
import torch.nn.functional as F

from ..data import get_dataloader
from ..engine.common import (GradDivergenceProbe, Meters,
                             build_optimizer, build_schedule,
                             decay_param_groups, progress_iter)
from ..models import build_model
from ..parallel import BucketedDataParallel
from ..profiling.metrics import (EpochMetrics, MetricsWriter,
                                 sample_gpu_resources, sample_host_resources)
from ..profiling.timers import StepProfiler
from ..runtime.distributed import (DistContext, barrier, setup_distributed,
                                   teardown_distributed)
from ..utils.seed import seed_everything


def _to_device(x, y, ctx: DistContext, augmenter=None):
    if ctx.is_gpu:
        x = x.to(ctx.device, non_blocking=True)
        if x.dtype == torch.uint8:  # raw loader: normalize on-device
            if augmenter is not None:
                x = augmenter(x)
            else:
                from ..data.cifar import normalize_uint8
                x = normalize_uint8(x)
        x = x.to(memory_format=torch.channels_last).to(torch.bfloat16)
        y = y.to(ctx.device, non_blocking=True)
    elif augmenter is not None:  # raw uint8 on CPU -> normalized f32
        x = augmenter(x)
    return x, y


def _make_augmenter(rank: int, pad: int, device):
    """Per-rank augmentation stream: ranks hold different shards, so the key
    mixes the rank into the shared seed."""
    from ..data.augment import DeviceAugment
    from ..utils.seed import DEFAULT_SEED
    return DeviceAugment((DEFAULT_SEED << 32) | rank, pad=pad, flip=True,
                         device=device)


def select_engine(engine: str, ctx: DistContext, model_name: str) -> str:
    """``auto`` → ``flat`` (hipGraph fast path) on GPU for models the flat
    manager supports, ``eager`` otherwise.  Explicit choices are honored
    (``flat`` on CPU raises — it is a GPU-only path by design)."""
    if engine == "auto":
        if ctx.is_gpu and model_name.lower().startswith(
                ("resnet", "mobilenet")):
            return "flat"
        return "eager"
    if engine == "flat" and not ctx.is_gpu:
        raise RuntimeError("--engine flat requires a GPU (hipGraph + HIP "
                           "extension path); use --engine eager on CPU")
    return engine


def train_dp_flat(ctx: DistContext, epochs: int, sample_size: int,
                  logs_dir: str, batch_size: int = 64,
                  model_name: str = "resnet18", lr: float = 1e-3,
                  optimizer_name: str = "adam",
                  synthetic: Optional[bool] = None, data_dir: str = "./data",
                  probe_divergence: bool = True, log_progress: bool = True,
                  use_graph: bool = True,
                  checkpoint_path: Optional[str] = None,
                  per_step_barrier: bool = False,
                  augment: bool = False, augment_pad: int = 4,
                  lr_schedule: str = "constant", warmup_epochs: float = 0.0,
                  min_lr: float = 0.0, lr_milestones=(), lr_gamma: float = 0.1,
                  weight_decay: float = 0.0, nesterov: bool = False,
                  decoupled_wd: bool = False, label_smoothing: float = 0.0,
                  no_decay_1d: bool = False, clip_grad_norm: float = 0.0,
                  lars: bool = False, lars_eta: float = 1e-3):
    """DP training on the flat fast path — the entrypoint-facing version of
    the bench.py flagship step (the parity entrypoint
    should run the best path we have).

    * flat f32 master / bf16 shadow params (``FlatParamManager``), fused
      Adam/SGD step, batched deferred wgrads;
    * the device-side step (normalize → forward → CE → backward → wgrad
      flush → pack → divergence probe [→ optimizer]) is captured in a
      hipGraph once and replayed per step, with the per-step H2D batch copy
      staged into static buffers outside the capture;
    * world>1: the bf16 gradient all-reduce runs EAGERLY between two
      captured graphs (fwd/bwd graph → RCCL all-reduce → optimizer graph).
      Keeping the collective out of the capture makes rank-divergent
      capture failures harmless (the collective sequence is identical in
      graph and eager modes) and gives an honest ``comm_time`` CSV column —
      the fully-captured single-graph variant (collective inside the graph,
      bucket-overlapped) is bench.py's flagship configuration;
    * loss/accuracy/divergence accumulate in static device scalars read
      once per epoch (no per-step sync); CSV schema unchanged.

    ``augment``: the normalize kernel is replaced by the fused random
    crop + flip + normalize kernel (plus a one-thread counter bump: one
    extra dispatch per step); its step counter
    lives on the device and advances under graph replay, and is set to
    ``start_epoch * len(loader)`` after the capture warm-ups so a resumed
    run continues the stream of an uninterrupted one.

    ``lr_schedule`` / ``warmup_epochs`` / ``min_lr`` / ``lr_milestones`` /
    ``lr_gamma`` (epochs, converted with ``len(loader)``): the schedule is
    built into the fused optimizer as a device table indexed by the device
    step counter, so the captured step walks it with no host work; the
    counter is reset after the capture warm-ups and positioned at
    ``start_epoch * len(loader)`` on a resume whose checkpoint carried none.
    ``weight_decay`` / ``nesterov`` / ``decoupled_wd`` (AdamW) reach the
    fused kernels, ``label_smoothing`` the fused cross-entropy.  All default
    to the unscheduled step, which launches the same kernels as before.

    ``no_decay_1d`` / ``clip_grad_norm`` / ``lars`` / ``lars_eta`` go to the
    Horizon optimizers, which then step through the segmented kernels; the
    norm reduction of clipping and LARS (2 dispatches) runs inside the
    captured optimizer step.  With world > 1 the norms are taken over the
    averaged gradient (the all-reduced bf16 buffer x 1/world) on every rank
    by the same fixed-order reduction, so replicas stay identical.

    Capture runs 3 warmup steps on the first batch shape; parameter /
    BN-buffer / optimizer state is snapshotted before and restored after,
    so training still starts from the seeded init.  Ragged final batches
    (shapes differing from the captured one) fall back to an eager step of
    the same math.
    """
    from .. import ops as _ops
    ext = _ops.extension()  # raises loudly if the HIP extension is missing
    from ..data.cifar import normalize_uint8
    from ..models._functional_gpu import cross_entropy
    from .flat import FlatParamManager, HorizonAdam, HorizonSGD

    rank, world = ctx.rank, ctx.world_size
    dev = ctx.device
    seed_everything(rank=0)  # identical replicas on every rank (no bcast)
    loader, sampler = get_dataloader(rank, world, batch_size, sample_size,
                                     strategy="dp", data_dir=data_dir,
                                     synthetic=synthetic, raw=True)
    model = build_model(model_name, num_classes=10).to(dev)
    mgr = FlatParamManager(model, dev)
    sched = build_schedule(lr_schedule, lr, epochs, len(loader),
                           warmup_epochs, min_lr, lr_milestones, lr_gamma)
    if lars and optimizer_name == "adam":
        raise ValueError("lars needs the sgd optimizer")
    opt = (HorizonAdam(mgr, lr=lr, weight_decay=weight_decay,
                       schedule=sched, decoupled_wd=decoupled_wd,
                       no_decay_1d=no_decay_1d,
                       clip_grad_norm=clip_grad_norm)
           if optimizer_name == "adam"
           else HorizonSGD(mgr, lr=lr, weight_decay=weight_decay,
                           schedule=sched, nesterov=nesterov,
                           no_decay_1d=no_decay_1d,
                           clip_grad_norm=clip_grad_norm, lars=lars,
                           lars_eta=lars_eta))
    import torch.distributed as dist
    force_comm = (os.environ.get("HZ_FORCE_COMM") == "1" and world == 1
                  and dist.is_initialized() and ctx.backend == "nccl")
    use_comm = (world > 1 and ctx.backend == "nccl") or force_comm
    comm_buf = (torch.zeros_like(mgr.grad, dtype=torch.bfloat16)
                if use_comm else None)
    inv_world = 1.0 / world
    augmenter = _make_augmenter(rank, augment_pad, dev) if augment else None
    to_norm = augmenter if augmenter is not None else normalize_uint8

    # static buffers + on-device accumulators
    sx = torch.empty(batch_size, 3, 32, 32, dtype=torch.uint8, device=dev)
    sy = torch.empty(batch_size, dtype=torch.int64, device=dev)
    loss_acc = torch.zeros((), device=dev)
    corr_acc = torch.zeros((), device=dev)
    prev = torch.zeros_like(mgr.grad) if probe_divergence else None
    sumsq = torch.zeros(1, device=dev) if probe_divergence else None
    div_acc = torch.zeros(1, device=dev) if probe_divergence else None

    # divergence probe fused into the optimizer kernel (Adam and SGD both
    # stream the f32 grad anyway — the standalone pass cost 61 us/step)
    fused_probe = probe_divergence
    probe_bufs = (prev, sumsq, div_acc) if fused_probe else None

    def fb_step(x_u8, y):
        """Capturable device-side step up to (not including) the optimizer:
        returns loss; leaves complete grads in mgr.grad and, when
        ``use_comm``, the bf16 pack in comm_buf."""
        x = to_norm(x_u8) \
            .to(memory_format=torch.channels_last).to(torch.bfloat16)
        logits = model(x)
        loss = cross_entropy(logits, y, label_smoothing)
        loss.backward()
        ext.flush_wgrad()  # batched deferred wgrads -> grads complete
        if use_comm:
            comm_buf.copy_(mgr.grad)  # pack f32 -> bf16 (half xGMI bytes)
        if probe_divergence and not fused_probe:
            ext.grad_divergence(mgr.grad, prev, sumsq, div_acc, False)
        loss_acc.add_(loss.detach() * y.shape[0])
        corr_acc.add_((logits.detach().argmax(1) == y).sum())
        return loss

    def opt_step():
        if use_comm:
            opt.step(grad_bf16=comm_buf, grad_scale=inv_world,
                     probe=probe_bufs)
        else:
            opt.step(probe=probe_bufs)

    # ---- hipGraph capture (state snapshotted/restored around it) --------
    graph_fb = graph_opt = None
    if use_graph:
        snap_master = mgr.master.detach().clone()
        snap_bufs = [(b, b.detach().clone()) for b in model.buffers()]
        g = torch.Generator(device="cpu").manual_seed(4321 + rank)
        sx.copy_(torch.randint(0, 256, sx.shape, dtype=torch.uint8,
                               generator=g))
        sy.copy_(torch.randint(0, 10, sy.shape, generator=g))
        try:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    loss = fb_step(sx, sy)
                    if use_comm:
                        dist.all_reduce(comm_buf)
                    opt_step()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            del loss
            if use_comm:
                # collective stays OUTSIDE the captures: fwd/bwd graph,
                # eager RCCL all-reduce, optimizer graph
                graph_fb = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph_fb):
                    fb_step(sx, sy)
                graph_opt = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph_opt):
                    opt_step()
            else:  # world=1: one whole-step graph
                graph_fb = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph_fb):
                    fb_step(sx, sy)
                    opt_step()
                graph_opt = None
        except Exception as e:  # noqa: BLE001 — eager fallback is safe:
            # the collective sequence is identical either way
            print(f"[dp-flat r{rank}] graph capture failed ({e!r}); "
                  "running eager flat steps", flush=True)
            graph_fb = graph_opt = None
        # restore seeded init state: capture warmups must not train
        with torch.no_grad():
            mgr.master.copy_(snap_master)
            mgr.shadow.copy_(mgr.master)
            for b, s in snap_bufs:
                b.copy_(s)
            mgr.grad.zero_()
            mgr.stats_arena.zero_()
            if isinstance(opt, HorizonAdam):
                opt.m.zero_(), opt.v.zero_()
            elif opt.mom is not None:
                opt.mom.zero_()
            opt.set_step(0)  # Adam's step_t, scheduled SGD's too
            loss_acc.zero_(), corr_acc.zero_()
            if probe_divergence:
                prev.zero_(), sumsq.zero_(), div_acc.zero_()
        mgr.refresh_rsck()
        del snap_master, snap_bufs
        torch.cuda.synchronize()

    # checkpoint/resume (addition over the reference):
    # restore AFTER capture so warmup/restore cannot clobber resumed state
    start_epoch = 0
    if checkpoint_path is not None and os.path.isfile(checkpoint_path):
        from ..utils.checkpoint import load_checkpoint
        state = load_checkpoint(checkpoint_path, model, opt, mgr=mgr)
        start_epoch = int(state.get("epoch", 0))
        if log_progress and rank == 0:
            print(f"[dp-flat] resumed from {checkpoint_path} "
                  f"(epoch {start_epoch})", flush=True)
        # a checkpoint from before SGD kept a step counter carries none
        if (sched is not None
                and state.get("optimizer", {}).get("step_t") is None):
            opt.set_step(start_epoch * len(loader))
    if augmenter is not None:  # the capture warm-ups advanced the counter
        augmenter.set_step(start_epoch * len(loader))

    prof = StepProfiler(dev)
    writer = MetricsWriter(logs_dir, rank, sample_size,
                           with_bandwidth=False, with_gpu=True)
    import psutil
    proc = psutil.Process()
    proc.cpu_percent(interval=None)

    count = 0
    for epoch in range(start_epoch, epochs):
        if sampler is not None:
            sampler.set_epoch(epoch)
        with prof.idle():
            barrier(ctx)
        epoch_start = time.time()
        cpu_samples, mem_samples = [], []
        n_steps = 0

        for x, y in progress_iter(loader, f"dp-flat r{rank} e{epoch + 1}",
                                  log_progress):
            prof.step_begin()
            cpu, mem = sample_host_resources(proc)
            cpu_samples.append(cpu)
            mem_samples.append(mem)
            if graph_fb is not None and x.shape[0] == batch_size:
                with prof.compute():
                    sx.copy_(x, non_blocking=True)
                    sy.copy_(y, non_blocking=True)
                    graph_fb.replay()
                if use_comm:
                    with prof.comm():
                        dist.all_reduce(comm_buf)
                        prof.add_bytes(comm_buf.numel()
                                       * comm_buf.element_size())
                if graph_opt is not None:
                    with prof.compute():
                        graph_opt.replay()
            else:  # eager step (capture failed, or ragged final batch)
                xg = x.to(dev, non_blocking=True)
                yg = y.to(dev, non_blocking=True)
                with prof.compute():
                    fb_step(xg, yg)
                if use_comm:
                    with prof.comm():
                        dist.all_reduce(comm_buf)
                        prof.add_bytes(comm_buf.numel()
                                       * comm_buf.element_size())
                with prof.compute():
                    opt_step()
            if per_step_barrier:  # reference data_parallel_train.py:150-152
                with prof.idle():
                    barrier(ctx)
            count += y.shape[0]
            n_steps += 1
            prof.step_end()

        t = prof.epoch_end()  # syncs: epoch_time includes the GPU tail
        epoch_time = time.time() - epoch_start
        loss_v = float(loss_acc.cpu()) / max(1, count)
        acc_v = 100.0 * float(corr_acc.cpu()) / max(1, count)
        div_v = (float(div_acc.cpu()) / max(1, n_steps)
                 if probe_divergence else 0.0)
        loss_acc.zero_(), corr_acc.zero_()
        if probe_divergence:
            div_acc.zero_()
        count = 0
        gmem, gutil = sample_gpu_resources(dev)
        m = EpochMetrics(
            epoch=epoch + 1, loss=loss_v, accuracy=acc_v,
            epoch_time=epoch_time, avg_step_time=t["avg_step_time"],
            compute_time=t["compute_time"], comm_time=t["comm_time"],
            idle_time=t["idle_time"],
            avg_cpu=sum(cpu_samples) / max(1, len(cpu_samples)),
            avg_memory=sum(mem_samples) / max(1, len(mem_samples)),
            grad_divergence=div_v, gpu_memory_mb=gmem, gpu_util=gutil)
        writer.append(m)
        if log_progress and rank == 0:
            print(f"[dp-flat rank0] epoch {epoch + 1}/{epochs} "
                  f"loss={loss_v:.4f} acc={acc_v:.2f}% "
                  f"time={epoch_time:.2f}s", flush=True)
        if checkpoint_path is not None and rank == 0:
            from ..utils.checkpoint import save_checkpoint
            save_checkpoint(checkpoint_path, model, opt, epoch=epoch + 1,
                            mgr=mgr)
        with prof.idle():
            barrier(ctx)
    return writer.path


def train_dp(ctx: DistContext, epochs: int, sample_size: int, logs_dir: str,
             batch_size: int = 64, model_name: str = "resnet18",
             lr: float = 1e-3, optimizer_name: str = "adam",
             synthetic: Optional[bool] = None, data_dir: str = "./data",
             probe_divergence: bool = True, log_progress: bool = True,
             checkpoint_path: Optional[str] = None,
             per_step_barrier: bool = False,
             augment: bool = False, augment_pad: int = 4,
             lr_schedule: str = "constant", warmup_epochs: float = 0.0,
             min_lr: float = 0.0, lr_milestones=(), lr_gamma: float = 0.1,
             weight_decay: float = 0.0, nesterov: bool = False,
             decoupled_wd: bool = False, label_smoothing: float = 0.0,
             no_decay_1d: bool = False, clip_grad_norm: float = 0.0,
             lars: bool = False, lars_eta: float = 1e-3):
    """Run the DP training loop for this rank; writes the per-worker CSV.

    ``no_decay_1d``: torch param groups from ``decay_param_groups``.
    ``clip_grad_norm`` (> 0): ``torch.nn.utils.clip_grad_norm_`` on the
    averaged gradient, between the all-reduce and the step.  ``lars``: the
    optimizer is ``engine.lars.LARS``.

    ``per_step_barrier=True`` restores the reference's full-world barrier
    after EVERY step (``data_parallel_train.py:150-152``) so ``idle_time``
    measures per-step peer skew exactly as the reference's does; the
    default barriers per epoch (a per-step barrier would dominate ~1 ms
    GPU steps — documented deviation)."""
    rank, world = ctx.rank, ctx.world_size
    seed_everything(rank=rank)
    loader, sampler = get_dataloader(rank, world, batch_size, sample_size,
                                     strategy="dp", data_dir=data_dir,
                                     synthetic=synthetic,
                                     raw=ctx.is_gpu or augment)
    augmenter = (_make_augmenter(rank, augment_pad,
                                 ctx.device if ctx.is_gpu else "cpu")
                 if augment else None)

    model = build_model(model_name, num_classes=10)
    if ctx.is_gpu:
        model = model.to(ctx.device)
    ddp = BucketedDataParallel(model, profiler=None)
    optimizer = build_optimizer(
        decay_param_groups(model, weight_decay) if no_decay_1d
        else model.parameters(), optimizer_name, lr=lr,
        weight_decay=weight_decay, nesterov=nesterov,
        decoupled_wd=decoupled_wd, lars=lars, lars_eta=lars_eta)
    sched = build_schedule(lr_schedule, lr, epochs, len(loader),
                           warmup_epochs, min_lr, lr_milestones, lr_gamma)
    probe = GradDivergenceProbe(model.parameters()) if probe_divergence else None

    prof = StepProfiler(ctx.device if ctx.is_gpu else None)
    ddp.profiler = prof
    writer = MetricsWriter(logs_dir, rank, sample_size,
                           with_bandwidth=False, with_gpu=ctx.is_gpu)
    meters = Meters(ctx.device if ctx.is_gpu else None)

    import psutil
    proc = psutil.Process()
    proc.cpu_percent(interval=None)  # prime

    start_epoch = 0
    if checkpoint_path is not None and os.path.isfile(checkpoint_path):
        from ..utils.checkpoint import load_checkpoint
        state = load_checkpoint(checkpoint_path, model, optimizer)
        start_epoch = int(state.get("epoch", 0))
        if log_progress and rank == 0:
            print(f"[dp] resumed from {checkpoint_path} "
                  f"(epoch {start_epoch})", flush=True)
    if augmenter is not None:
        augmenter.set_step(start_epoch * len(loader))

    for epoch in range(start_epoch, epochs):
        if sampler is not None:
            sampler.set_epoch(epoch)
        with prof.idle():
            barrier(ctx)
        epoch_start = time.time()
        cpu_samples, mem_samples = [], []

        for step, (x, y) in enumerate(progress_iter(
                loader, f"dp r{rank} e{epoch + 1}", log_progress)):
            prof.step_begin()
            cpu, mem = sample_host_resources(proc)
            cpu_samples.append(cpu)
            mem_samples.append(mem)

            x, y = _to_device(x, y, ctx, augmenter)
            if sched is not None:  # same table the flat engine indexes
                lr_t = sched.lr_at(epoch * len(loader) + step)
                for group in optimizer.param_groups:
                    group["lr"] = lr_t
            with prof.compute():
                optimizer.zero_grad(set_to_none=True)
                logits = ddp(x)
                if logits.is_cuda:
                    from ..models._functional_gpu import cross_entropy
                    loss = cross_entropy(logits, y, label_smoothing)
                else:
                    loss = F.cross_entropy(logits.float(), y,
                                           label_smoothing=label_smoothing)
                loss.backward()
            with prof.comm():
                ddp.finalize_backward()
            with prof.compute():
                if clip_grad_norm > 0:
                    torch.nn.utils.clip_grad_norm_(model.parameters(),
                                                   clip_grad_norm)
                optimizer.step()
                if ctx.is_gpu:
                    from ..models import refresh_all_shadows
                    refresh_all_shadows(model)
            meters.update(loss, logits, y)
            if probe is not None:
                probe.step()
            if per_step_barrier:  # reference data_parallel_train.py:150-152
                with prof.idle():
                    barrier(ctx)
            prof.step_end()

        t = prof.epoch_end()  # syncs: epoch_time includes the GPU tail
        epoch_time = time.time() - epoch_start
        loss_v, acc_v = meters.epoch_values()
        gmem, gutil = sample_gpu_resources(ctx.device if ctx.is_gpu else None)
        m = EpochMetrics(
            epoch=epoch + 1, loss=loss_v, accuracy=acc_v,
            epoch_time=epoch_time, avg_step_time=t["avg_step_time"],
            compute_time=t["compute_time"], comm_time=t["comm_time"],
            idle_time=t["idle_time"],
            avg_cpu=sum(cpu_samples) / max(1, len(cpu_samples)),
            avg_memory=sum(mem_samples) / max(1, len(mem_samples)),
            grad_divergence=probe.epoch_value() if probe is not None else 0.0,
            gpu_memory_mb=gmem, gpu_util=gutil)
        writer.append(m)
        if log_progress and rank == 0:
            print(f"[dp rank0] epoch {epoch + 1}/{epochs} "
                  f"loss={loss_v:.4f} acc={acc_v:.2f}% "
                  f"time={epoch_time:.2f}s", flush=True)
        if checkpoint_path is not None and rank == 0:
            from ..utils.checkpoint import save_checkpoint
            save_checkpoint(checkpoint_path, model, optimizer,
                            epoch=epoch + 1)
        with prof.idle():
            barrier(ctx)
    return writer.path


def dp_worker(rank: int, world_size: int, epochs: int, sample_size: int,
              port: int, logs_dir: str, batch_size: int = 64,
              model_name: str = "resnet18", backend: Optional[str] = None,
              synthetic: Optional[bool] = None, lr: float = 1e-3,
              optimizer_name: str = "adam", engine: str = "auto",
              checkpoint_path: Optional[str] = None,
              per_step_barrier: bool = False,
              augment: bool = False, augment_pad: int = 4,
              lr_schedule: str = "constant", warmup_epochs: float = 0.0,
              min_lr: float = 0.0, lr_milestones=(), lr_gamma: float = 0.1,
              weight_decay: float = 0.0, nesterov: bool = False,
              decoupled_wd: bool = False, label_smoothing: float = 0.0,
              no_decay_1d: bool = False, clip_grad_norm: float = 0.0,
              lars: bool = False, lars_eta: float = 1e-3):
    """Spawned worker entry (reference ``data_parallel_train.py:192-230``).

    ``engine``: ``flat`` (default on GPU via ``auto``) runs the hipGraph /
    fused-step fast path; ``eager`` the bucketed-DDP torch-optimizer loop.
    ``checkpoint_path``: save per epoch (rank 0) and resume when the file
    exists — an extension over the reference.
    The schedule / weight-decay / Nesterov / AdamW / label-smoothing /
    no-decay / clipping / LARS knobs go to whichever engine runs (see
    ``train_dp_flat``)."""
    ctx = setup_distributed(rank, world_size, port, backend=backend)
    try:
        if ctx.is_gpu and model_name.startswith("resnet"):
            # fail loudly if the native extension is missing on a GPU box
            from .. import ops as _ops
            _ops.extension()
        eng = select_engine(engine, ctx, model_name)
        if eng == "flat":
            train_dp_flat(ctx, epochs, sample_size, logs_dir,
                          batch_size=batch_size, model_name=model_name,
                          synthetic=synthetic, lr=lr,
                          optimizer_name=optimizer_name,
                          checkpoint_path=checkpoint_path,
                          per_step_barrier=per_step_barrier,
                          augment=augment, augment_pad=augment_pad,
                          lr_schedule=lr_schedule, warmup_epochs=warmup_epochs,
                          min_lr=min_lr, lr_milestones=lr_milestones,
                          lr_gamma=lr_gamma, weight_decay=weight_decay,
                          nesterov=nesterov, decoupled_wd=decoupled_wd,
                          label_smoothing=label_smoothing,
                          no_decay_1d=no_decay_1d,
                          clip_grad_norm=clip_grad_norm, lars=lars,
                          lars_eta=lars_eta)
        else:
            train_dp(ctx, epochs, sample_size, logs_dir,
                     batch_size=batch_size, model_name=model_name,
                     synthetic=synthetic, lr=lr,
                     optimizer_name=optimizer_name,
                     checkpoint_path=checkpoint_path,
                     per_step_barrier=per_step_barrier,
                     augment=augment, augment_pad=augment_pad,
                     lr_schedule=lr_schedule, warmup_epochs=warmup_epochs,
                     min_lr=min_lr, lr_milestones=lr_milestones,
                     lr_gamma=lr_gamma, weight_decay=weight_decay,
                     nesterov=nesterov, decoupled_wd=decoupled_wd,
                     label_smoothing=label_smoothing,
                     no_decay_1d=no_decay_1d, clip_grad_norm=clip_grad_norm,
                     lars=lars, lars_eta=lars_eta)
    finally:
        teardown_distributed(ctx)
