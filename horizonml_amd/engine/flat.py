"""Flat parameter/gradient management for the MI355X fast path.

MI355X-first memory design (288 GB HBM3E: keep everything resident, few big
buffers, single-kernel updates):

* ONE flat f32 master buffer holds every trainable parameter (modules' params
  are re-pointed to views), ONE flat f32 gradient buffer (``.grad`` views are
  pre-assigned so autograd accumulates in place — stable addresses under
  hipGraph capture), ONE flat bf16 shadow the conv/linear kernels consume.
* The fused Adam/SGD kernel updates master + emits the bf16
  shadow + zeroes the gradient buffer in a single pass over the flat range.
* dgrad reads the KRSC shadow directly (transposed LDS read).  Only with
  ``HZ_DGRAD_KRSC=0`` / ``set_dgrad_krsc(False)`` does a second flat bf16
  buffer hold RSCK weight images, refreshed by one batched permute kernel
  per step.
* DP gradient sync becomes ONE bf16 all-reduce of the flat buffer.
* Anything that depends on which parameter an element belongs to (no weight
  decay on 1-D parameters, global-norm clipping, the LARS trust ratio) goes
  through a segment table: one segment per parameter, cut into chunks of at
  most ``SEG_CHUNK`` elements, one workgroup per chunk (docs/KERNELS.md,
  "Segmented step").  Built only when an optimizer asks for it.
* Filter taps that only ever meet padding (ResNet18 at 32x32: 62 % of the
  buffer) have a zero gradient for good; without weight decay the step is the
  identity on them.  The manager keeps a chunk table of the live ranges,
  built from the native tap-window registry and verified against the device
  state, and the unsegmented decay-free step streams only those
  (docs/KERNELS.md, "Live-range step").
"""
from __future__ import annotations

from typing import List

import torch
import torch.nn as nn

from .. import ops as _ops
from ..models.layers import ConvBNAct, DepthwiseConvBNAct, Linear


SEG_CHUNK = 4096  # elements per chunk = per workgroup of the *_seg kernels


class SegmentTable:
    """Device tables of a segmented flat buffer.

    ``sizes[s]`` elements per segment, in buffer order; ``decay[s]`` /
    ``adapt[s]`` the contract's static flags.  ``chunks`` int32
    ``[nchunks, 3] = (segment, start, length)`` with ``length <= chunk`` and
    no chunk crossing a segment; ``seg_meta`` int32 ``[nseg, 3] = (first
    chunk, one past the last chunk, decay | adapt << 1)``.  Both are correct
    by construction: the kernels index the flat buffers with them unchecked."""

    def __init__(self, sizes, decay, adapt, device, chunk: int = SEG_CHUNK):
        sizes = [int(n) for n in sizes]
        if not sizes or min(sizes) < 1 or chunk < 1:
            raise ValueError("segments must be non-empty")
        if not len(sizes) == len(decay) == len(adapt):
            raise ValueError("one decay and one adapt flag per segment")
        if sum(sizes) >= 2 ** 31:
            raise ValueError("segment offsets are int32")
        chunks, meta, bounds = [], [], [0]
        for s, n in enumerate(sizes):
            b, c0 = bounds[-1], len(chunks)
            for o in range(0, n, chunk):
                chunks.append((s, b + o, min(chunk, n - o)))
            meta.append((c0, len(chunks),
                         int(bool(decay[s])) | int(bool(adapt[s])) << 1))
            bounds.append(b + n)
        self.sizes, self.bounds = sizes, bounds
        self.decay = [bool(d) for d in decay]
        self.adapt = [bool(a) for a in adapt]
        self.numel, self.nseg, self.nchunks = bounds[-1], len(sizes), len(chunks)
        self.chunks = torch.tensor(chunks, dtype=torch.int32, device=device)
        self.seg_meta = torch.tensor(meta, dtype=torch.int32, device=device)

    def static_mul(self, wd: float) -> torch.Tensor:
        """``seg_mul`` with nothing data-dependent in it: ``(1, wd*decay_s)``."""
        return torch.tensor([(1.0, wd if d else 0.0) for d in self.decay],
                            dtype=torch.float32, device=self.chunks.device)


class _SegState:
    """What a Horizon optimizer holds once it steps through the segmented
    kernels: the table, ``seg_mul`` and, with clipping or LARS, the buffers
    of the per-step norm reduction."""

    def __init__(self, mgr, wd, no_decay_1d, max_norm, lars, eta):
        self.table = t = mgr.segment_table(no_decay_1d)
        self.wd, self.max_norm = float(wd), float(max_norm)
        self.lars, self.eta = bool(lars), float(eta)
        self.seg_mul = t.static_mul(self.wd)
        self.dynamic = self.max_norm > 0 or self.lars
        if self.dynamic:
            dev = mgr.master.device
            self.partials = torch.zeros(t.nchunks, 2, device=dev)
            self.seg_norms = torch.zeros(t.nseg, 2, device=dev)
            self.norm_out = torch.zeros(2, device=dev)

    def reduce(self, ext, mgr, grad_bf16, grad_scale):
        """partials + finalize: 2 dispatches, refills ``seg_mul``."""
        if self.dynamic:
            ext.seg_norms(mgr.master, mgr.grad, self.table.chunks,
                          self.table.seg_meta, self.partials, self.seg_norms,
                          self.seg_mul, self.norm_out, self.wd, self.max_norm,
                          self.lars, self.eta, grad_bf16, grad_scale)

    def last_grad_norm(self) -> float:
        if not self.dynamic:
            raise RuntimeError("the gradient norm is only computed with "
                               "clip_grad_norm > 0 or lars")
        return float(self.norm_out[0].cpu())


LIVE_CHUNK = 4096  # elements per chunk = per workgroup of the *_live kernels


def build_live_chunks(numel, windows, chunk: int = LIVE_CHUNK):
    """Chunk table of the live part of a flat buffer of ``numel`` elements.

    ``windows``: ``(offset, K, Rf, Sf, C, r0, R, s0, S)`` per conv weight —
    a KRSC filter ``[K, Rf, Sf, C]`` at ``offset`` whose taps outside rows
    ``[r0, r0+R)`` × columns ``[s0, s0+S)`` are dead.  Everything else of the
    buffer is live, and live spans run across parameter boundaries.

    Returns ``(chunks, n_dead)``: ``chunks`` a list of ``(start, run_len,
    run_pitch, nruns)`` — elements ``start + r*run_pitch + j`` for
    ``r < nruns``, ``j < run_len``, at most ``chunk`` of them — that covers
    every live element exactly once and no dead one.  A clipped filter's live
    elements are, per window row, K runs of ``S*C`` at pitch ``Rf*Sf*C`` (one
    run of ``R*Sf*C`` per filter when the window spans the filter's width);
    a chunk groups as many whole runs as fit, and a run longer than a chunk
    is cut.  Every chunk is checked against ``numel`` here, on the host: the
    kernels index the flat buffers with the table unchecked."""
    numel, chunk = int(numel), int(chunk)
    if numel < 1 or numel >= 2 ** 31 or chunk < 1:
        raise ValueError("live table offsets are int32")
    spans, families, cursor, n_dead = [], [], 0, 0
    for off, K, Rf, Sf, C, r0, R, s0, S in sorted(
            tuple(int(x) for x in w) for w in windows):
        kdf = Rf * Sf * C
        if min(K, Rf, Sf, C, R, S) < 1 or min(r0, s0) < 0 \
                or r0 + R > Rf or s0 + S > Sf:
            raise ValueError("tap window outside its filter")
        if off < cursor or off + K * kdf > numel:
            raise ValueError("conv weights overlap or leave the buffer")
        if R == Rf and S == Sf:
            continue  # fully live: stays inside the surrounding span
        if off > cursor:
            spans.append((cursor, off))
        cursor = off + K * kdf
        n_dead += K * (Rf * Sf - R * S) * C
        if S == Sf:
            families.append((off + r0 * Sf * C, R * Sf * C, kdf, K))
        else:
            families += [(off + ((r0 + r) * Sf + s0) * C, S * C, kdf, K)
                         for r in range(R)]
    if cursor < numel:
        spans.append((cursor, numel))

    chunks = []

    def cut(lo, hi):
        chunks.extend((o, min(chunk, hi - o), 0, 1)
                      for o in range(lo, hi, chunk))

    for lo, hi in spans:
        cut(lo, hi)
    for start, run_len, pitch, nruns in families:
        if run_len >= chunk or nruns == 1:
            for r in range(nruns):
                cut(start + r * pitch, start + r * pitch + run_len)
            continue
        group = chunk // run_len
        chunks.extend((start + r * pitch, run_len, pitch,
                       min(group, nruns - r))
                      for r in range(0, nruns, group))
    for start, run_len, pitch, nruns in chunks:
        if not (run_len >= 1 and nruns >= 1 and run_len * nruns <= chunk
                and start >= 0 and pitch >= 0
                and (nruns == 1 or pitch >= run_len)
                and start + (nruns - 1) * pitch + run_len <= numel):
            raise AssertionError("live chunk out of bounds")
    return chunks, n_dead


class _LiveTable:
    """The manager's live table and what it was built from: the registry
    version, and the per-element buffers (optimizer state, probe ``prev``,
    bf16 gradient) whose dead elements were verified zero at that build."""

    def __init__(self):
        self.version = -1          # -1: not built, or invalidated
        self.bufs = []             # verified at the last build
        self.chunks = None         # int32 [nchunks, 4] on the device, or None
        self.n_dead = 0
        self.n_demoted = 0         # clipped convs that failed the check
        self.nchunks = 0

    def covers(self, bufs):
        have = {t.data_ptr() for t in self.bufs}
        return all(t.data_ptr() in have for t in bufs)


def _seg_state(mgr, wd, no_decay_1d, max_norm, lars=False, eta=1e-3):
    if max_norm < 0 or eta <= 0:
        raise ValueError("clip_grad_norm must be >= 0 and lars_eta > 0")
    if not (no_decay_1d or max_norm > 0 or lars):
        return None
    return _SegState(mgr, wd, no_decay_1d, max_norm, lars, eta)


class FlatParamManager:
    def __init__(self, model: nn.Module, device: torch.device):
        self._seg_tables = {}
        # managed convs defer their weight-grad GEMMs: flush_wgrad() (called
        # by the fused optimizer step) runs them as one batched kernel
        _ops.extension().set_wgrad_defer(True)
        params = [p for p in model.parameters() if p.requires_grad]
        total = sum(p.numel() for p in params)
        self.params = params
        self.numel = total
        self.master = torch.zeros(total, device=device)
        self.grad = torch.zeros(total, device=device)
        # tap windows recorded at these addresses belong to a freed model
        _ops.extension().tap_window_reset(
            self.grad.data_ptr(), self.grad.data_ptr() + 4 * total)
        self.shadow = torch.zeros(total, device=device, dtype=torch.bfloat16)
        self.slices = {}
        off = 0
        for p in params:
            n = p.numel()
            with torch.no_grad():
                self.master[off:off + n].copy_(p.data.flatten())
            p.data = self.master[off:off + n].view(p.shape)
            p.grad = self.grad[off:off + n].view(p.shape)
            self.slices[id(p)] = (off, n)
            off += n
        with torch.no_grad():
            self.shadow.copy_(self.master)

        # wire bf16 shadow views into the modules; collect conv RSCK metadata
        convs = []
        for m in model.modules():
            if isinstance(m, (ConvBNAct, Linear, DepthwiseConvBNAct)):
                woff, wn = self.slices[id(m.weight)]
                m.weight_bf16 = self.shadow[woff:woff + wn].view(
                    m.weight.shape)
                m._managed = True
                if isinstance(m, ConvBNAct):
                    convs.append((m, woff, wn))
        # BN-stats arena: one pre-zeroed f32 slab per conv ([2K] each),
        # re-zeroed by the fused optimizer kernel each step (no per-conv
        # fill kernels in the forward).
        # conv weights by offset: what a tap-window registry entry must match
        # to count for this manager (live table, below)
        self._conv_shapes = {woff: tuple(m.weight.shape)
                             for m, woff, _ in convs}
        self._live = _LiveTable()
        stats_total = sum(2 * m.out_ch for m, _, _ in convs)
        self.stats_arena = torch.zeros(max(1, stats_total), device=device)
        soff = 0
        for m, _, _ in convs:
            m._stats_buf = self.stats_arena[soff:soff + 2 * m.out_ch]
            soff += 2 * m.out_ch

        # KRSC-direct dgrad (the default) reads the shadow itself: no RSCK
        # image, no per-step permute.  ``rsck`` stays a (0-element) tensor
        # so state snapshots and checkpoints treat both modes alike.
        self.meta = None
        self.max_elem = 1
        if _ops.extension().dgrad_krsc_enabled():
            self.rsck = torch.zeros(0, device=device, dtype=torch.bfloat16)
            for m, _, _ in convs:
                if hasattr(m, "_w_rsck"):  # left by an earlier manager
                    del m._w_rsck
            return
        rsck_total = sum(wn for _, _, wn in convs)
        self.rsck = torch.zeros(rsck_total, device=device,
                                dtype=torch.bfloat16)
        meta: List[List[int]] = []
        doff = 0
        self.max_elem = 1
        for m, woff, wn in convs:
            K, R, S, C = m.weight.shape
            meta.append([woff, doff, wn, (K << 16) | C])
            m._w_rsck = self.rsck[doff:doff + wn].view(R, S, C, K)
            doff += wn
            self.max_elem = max(self.max_elem, wn)
        self.meta = (torch.tensor(meta, dtype=torch.int32, device=device)
                     if meta else None)
        self.refresh_rsck()

    def refresh_rsck(self):
        """Rebuild the RSCK images from the shadow (legacy dgrad layout);
        launches nothing when the manager keeps no image."""
        if self.meta is not None:
            _ops.extension().permute_krsc_rsck(self.shadow, self.rsck,
                                               self.meta, self.max_elem)

    def zero_grad(self):
        self.grad.zero_()

    def segment_table(self, no_decay_1d: bool = False) -> SegmentTable:
        """One segment per parameter, in buffer order.  ``adapt_s = 0`` for
        ``ndim <= 1`` (BN weight/bias, linear/conv biases; depthwise conv
        weights are not); ``decay_s = 0`` for the same class when
        ``no_decay_1d``.  Built on first use and kept."""
        key = bool(no_decay_1d)
        if key not in self._seg_tables:
            one_d = [p.ndim <= 1 for p in self.params]
            self._seg_tables[key] = SegmentTable(
                [p.numel() for p in self.params],
                [not (key and d) for d in one_d], [not d for d in one_d],
                self.master.device)
        return self._seg_tables[key]

    # -- live table: the fused step skips dead filter taps -------------------
    def live_windows(self):
        """``(offset, K, Rf, Sf, C, r0, R, s0, S)`` of every conv weight of
        this manager the native tap-window registry knows, by offset.  An
        entry counts only when its pointer is a conv weight's gradient view
        of this manager and the filter shape agrees; a conv without one is
        fully live."""
        base, out = self.grad.data_ptr(), []
        for ptr, K, Rf, Sf, C, r0, R, s0, S in \
                _ops.extension().tap_window_registry():
            off, rem = divmod(ptr - base, 4)
            if rem == 0 and self._conv_shapes.get(off) == (K, Rf, Sf, C):
                out.append((off, K, Rf, Sf, C, r0, R, s0, S))
        return sorted(out)

    def invalidate_live_table(self):
        """The next eager ``step`` rebuilds (and re-verifies) the table; a
        captured one launches the full-range kernel until then."""
        self._live.version = -1

    def live_table_info(self):
        """State of the live table: ``state`` is ``"unbuilt"``, ``"none"``
        (built, no dead element: the full-range kernels run) or ``"live"``;
        ``skipped`` elements per step, ``nchunks``, and ``demoted``, the
        clipped convs kept fully live because their dead state was not
        zero."""
        lt = self._live
        state = ("unbuilt" if lt.version < 0
                 else "none" if lt.chunks is None else "live")
        return {"state": state, "version": lt.version,
                "skipped": lt.n_dead if state == "live" else 0,
                "nchunks": lt.nchunks if state == "live" else 0,
                "demoted": lt.n_demoted}

    def live_chunks(self, bufs):
        """The live table for a step that streams ``bufs`` (optimizer state,
        probe ``prev``, bf16 gradient; ``None`` entries ignored) besides
        master, grad and shadow — or ``None`` when the step must launch the
        full-range kernel: switched off, nothing dead, or stale while the
        stream is capturing.  Stale outside capture: rebuilt here."""
        ext = _ops.extension()
        if not ext.opt_skip_dead_enabled():
            return None
        lt = self._live
        bufs = [t for t in bufs if t is not None]
        version = ext.tap_window_version()
        if lt.version != version or not lt.covers(bufs):
            if torch.cuda.is_current_stream_capturing():
                return None
            have = {t.data_ptr() for t in bufs}
            bufs += [t for t in lt.bufs if t.data_ptr() not in have]
            self._build_live_table(version, bufs)
        return lt.chunks

    def _build_live_table(self, version, bufs):
        """Not in the hot loop: one reduction with one host sync verifies
        the identity precondition on the device state itself — grad and
        every buffer of ``bufs`` hold the bit pattern of +0 on every dead
        element (so g = m = v = 0 there and, without weight decay, the
        update is the identity).  A conv that fails is kept fully live.
        Then shadow = bf16(master) over the whole buffer, once: the skipped
        elements hold what the full kernel would have written."""
        lt = self._live
        wins = self.live_windows()
        clipped = [w for w in wins if w[6] * w[8] < w[2] * w[3]]
        lt.n_demoted = 0
        if clipped:
            counts = []
            for off, K, Rf, Sf, C, r0, R, s0, S in clipped:
                n, c = K * Rf * Sf * C, 0
                for t in [self.grad] + bufs:
                    bits = t[off:off + n].view(
                        torch.int32 if t.element_size() == 4 else torch.int16
                    ).view(K, Rf, Sf, C)
                    c = c + torch.count_nonzero(bits) - torch.count_nonzero(
                        bits[:, r0:r0 + R, s0:s0 + S])
                counts.append(c)
            bad = torch.stack(counts).cpu().tolist()
            lt.n_demoted = sum(1 for b in bad if b)
            clipped = [w for w, b in zip(clipped, bad) if not b]
        chunks, lt.n_dead = build_live_chunks(self.numel, clipped)
        if lt.n_dead:
            lt.chunks = torch.tensor(chunks, dtype=torch.int32,
                                     device=self.master.device)
            lt.nchunks = len(chunks)
            with torch.no_grad():
                self.shadow.copy_(self.master)
        else:
            lt.chunks, lt.nchunks = None, 0
        lt.version, lt.bufs = version, bufs


def _sched_buffers(schedule, dev):
    """Device residents of a scheduled optimizer: the f32 lr table the kernel
    indexes with its step counter, and the scalar it records the lr in."""
    if schedule is None:
        return None, None
    return schedule.table().to(dev), torch.zeros(1, device=dev)


class HorizonAdam:
    """Fused flat-buffer Adam (K9): 1 elementwise kernel + step increment
    per step (+ the batched RSCK permute in the legacy dgrad layout);
    zero_grad folded in.

    ``schedule`` (an ``LRSchedule``): the learning rate of update ``t`` is
    read on the device from the schedule's table, indexed by ``step_t`` — a
    captured step walks the schedule under graph replay, and ``lr`` is
    unused.  ``decoupled_wd``: AdamW (``w *= 1 - lr*wd`` instead of
    ``g += wd*w``).  With neither, ``step`` launches ``k_adam_step`` as
    before.

    ``no_decay_1d``: no weight decay on ``ndim <= 1`` parameters.
    ``clip_grad_norm`` (> 0): scale the gradient so its global L2 norm is at
    most this, ``torch.nn.utils.clip_grad_norm_``'s definition; the norm is
    reduced on the device inside the step (2 added dispatches).  Either one
    routes ``step`` through ``k_adam_step_seg``; with neither, nothing is
    allocated and the branches above run as they are."""

    def __init__(self, mgr: FlatParamManager, lr: float = 1e-3,
                 betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, schedule=None,
                 decoupled_wd: bool = False, no_decay_1d: bool = False,
                 clip_grad_norm: float = 0.0):
        self.mgr = mgr
        self.seg = _seg_state(mgr, weight_decay, no_decay_1d, clip_grad_norm)
        self.lr, self.betas, self.eps, self.wd = lr, betas, eps, weight_decay
        self.schedule, self.decoupled = schedule, bool(decoupled_wd)
        dev = mgr.master.device
        self.m = torch.zeros_like(mgr.master)
        self.v = torch.zeros_like(mgr.master)
        self.step_t = torch.zeros(1, device=dev)
        self.lr_table, self.lr_out = _sched_buffers(schedule, dev)
        self._live_stale = False  # set by load_state_dict

    def step(self, zero_grad: bool = True, grad_bf16=None,
             grad_scale: float = 1.0, probe=None):
        """``grad_bf16``: consume an all-reduced bf16 gradient buffer
        directly (× ``grad_scale``) — skips the DP unpack pass.
        ``probe``: optional ``(prev, sumsq, out)`` f32 tensors — the
        grad-divergence probe fused into the Adam pass (the standalone
        kernel costs a 3×|grad| extra sweep per step)."""
        ext = _ops.extension()
        ext.flush_wgrad()  # batched deferred weight grads
        p0, p1, p2 = probe if probe is not None else (None, None, None)
        if self._live_stale:
            self.mgr.invalidate_live_table()
            self._live_stale = False
        if self.seg is not None:
            self.seg.reduce(ext, self.mgr, grad_bf16, grad_scale)
            ext.adam_step_seg(self.mgr.master, self.mgr.grad, self.m, self.v,
                              self.mgr.shadow, self.step_t, self.lr_table,
                              self.lr_out, self.lr, self.betas[0],
                              self.betas[1], self.eps, self.decoupled,
                              zero_grad, self.seg.table.chunks,
                              self.seg.seg_mul, self.mgr.stats_arena,
                              grad_bf16, grad_scale, p0, p1, p2)
        elif self.wd == 0 and (live := self.mgr.live_chunks(
                (self.m, self.v, p0, grad_bf16))) is not None:
            # no decay of either kind: dead filter taps keep their value,
            # only the live ranges are streamed (k_adam_step_live)
            ext.adam_step_live(self.mgr.master, self.mgr.grad, self.m,
                               self.v, self.mgr.shadow, self.step_t,
                               self.lr_table, self.lr_out, self.lr,
                               self.betas[0], self.betas[1], self.eps,
                               zero_grad, live, self.mgr.stats_arena,
                               grad_bf16, grad_scale, p0, p1, p2)
        elif self.schedule is None and not self.decoupled:
            ext.adam_step(self.mgr.master, self.mgr.grad, self.m,
                          self.v, self.mgr.shadow, self.step_t,
                          self.lr, self.betas[0], self.betas[1],
                          self.eps, self.wd, zero_grad,
                          self.mgr.stats_arena, grad_bf16,
                          grad_scale, p0, p1, p2)
        else:
            ext.adam_step_sched(self.mgr.master, self.mgr.grad, self.m,
                                self.v, self.mgr.shadow, self.step_t,
                                self.lr_table, self.lr_out, self.lr,
                                self.betas[0], self.betas[1], self.eps,
                                self.wd, self.decoupled, zero_grad,
                                self.mgr.stats_arena, grad_bf16, grad_scale,
                                p0, p1, p2)
        self.mgr.refresh_rsck()

    def current_lr(self) -> float:
        """The learning rate the last update used.  Syncs — not for the hot
        loop."""
        if self.lr_out is None:
            return float(self.lr)
        return float(self.lr_out.cpu())

    def last_grad_norm(self) -> float:
        """Global L2 norm of the gradient the last update saw, before
        clipping.  Syncs — not for the hot loop."""
        if self.seg is None:
            raise RuntimeError("the gradient norm is only computed with "
                               "clip_grad_norm > 0 or lars")
        return self.seg.last_grad_norm()

    def set_step(self, n: int):
        """Position the update counter: the next ``step`` is update ``n``
        (0-based) — it reads ``lr_at(n)`` and bias-corrects with ``n + 1``."""
        self.step_t.fill_(float(n))

    # -- checkpoint round-trip (utils/checkpoint.py) ----------------------
    def state_dict(self):
        return {"kind": "horizon_adam", "lr": self.lr, "betas": self.betas,
                "eps": self.eps, "weight_decay": self.wd,
                "m": self.m.detach().cpu(), "v": self.v.detach().cpu(),
                "step_t": self.step_t.detach().cpu()}

    def load_state_dict(self, state):
        if state.get("kind") != "horizon_adam":
            raise ValueError("checkpoint optimizer state is not HorizonAdam")
        self._live_stale = True  # loaded moments: verify the table again
        with torch.no_grad():
            self.m.copy_(state["m"].to(self.m.device))
            self.v.copy_(state["v"].to(self.v.device))
            self.step_t.copy_(state["step_t"].to(self.step_t.device))


class HorizonSGD:
    """Fused flat-buffer SGD.  ``schedule``: as for ``HorizonAdam``; SGD then
    owns an f32 device ``step_t``, bumped by a one-thread kernel in front of
    the update (one added dispatch per step).  ``nesterov``: torch's
    definition (``w -= lr*(g + mu*u)``).  With neither, ``step`` launches
    ``k_sgd_step`` alone as before.

    ``no_decay_1d`` / ``clip_grad_norm``: as for ``HorizonAdam``.  ``lars``:
    layer-wise trust ratio ``lars_eta*|w| / (|g| + wd*|w| + 1e-8)`` on every
    ``ndim > 1`` parameter (``engine.lars.LARS`` is the same contract in
    plain torch).  Any of them routes ``step`` through ``k_sgd_step_seg``;
    clipping and LARS add the 2-dispatch norm reduction in front of it."""

    def __init__(self, mgr: FlatParamManager, lr: float = 0.1,
                 momentum: float = 0.9, weight_decay: float = 0.0,
                 schedule=None, nesterov: bool = False,
                 no_decay_1d: bool = False, clip_grad_norm: float = 0.0,
                 lars: bool = False, lars_eta: float = 1e-3):
        if nesterov and not momentum > 0:
            raise ValueError("nesterov needs momentum > 0")
        self.mgr = mgr
        self.seg = _seg_state(mgr, weight_decay, no_decay_1d, clip_grad_norm,
                              lars, lars_eta)
        self.lr, self.mu, self.wd = lr, momentum, weight_decay
        self.schedule, self.nesterov = schedule, bool(nesterov)
        self.mom = (torch.zeros_like(mgr.master) if momentum > 0 else None)
        dev = mgr.master.device
        self.lr_table, self.lr_out = _sched_buffers(schedule, dev)
        self.step_t = (torch.zeros(1, device=dev)
                       if schedule is not None else None)
        self._live_stale = False  # set by load_state_dict

    def step(self, zero_grad: bool = True, grad_bf16=None,
             grad_scale: float = 1.0, probe=None):
        """``probe``: optional ``(prev, sumsq, out)`` — the divergence
        probe fused into the SGD pass, like HorizonAdam's."""
        ext = _ops.extension()
        ext.flush_wgrad()  # batched deferred weight grads
        p0, p1, p2 = probe if probe is not None else (None, None, None)
        if self._live_stale:
            self.mgr.invalidate_live_table()
            self._live_stale = False
        if self.seg is not None:
            self.seg.reduce(ext, self.mgr, grad_bf16, grad_scale)
            ext.sgd_step_seg(self.mgr.master, self.mgr.grad, self.mom,
                             self.mgr.shadow, self.step_t, self.lr_table,
                             self.lr_out, self.lr, self.mu, self.nesterov,
                             zero_grad, self.seg.table.chunks,
                             self.seg.seg_mul, grad_bf16, grad_scale,
                             p0, p1, p2)
        elif self.wd == 0 and (live := self.mgr.live_chunks(
                (self.mom, p0, grad_bf16))) is not None:
            ext.sgd_step_live(self.mgr.master, self.mgr.grad, self.mom,
                              self.mgr.shadow, self.step_t, self.lr_table,
                              self.lr_out, self.lr, self.mu, self.nesterov,
                              zero_grad, live, grad_bf16, grad_scale,
                              p0, p1, p2)
        elif self.schedule is None and not self.nesterov:
            ext.sgd_step(self.mgr.master, self.mgr.grad, self.mom,
                         self.mgr.shadow, self.lr, self.mu, self.wd,
                         zero_grad, grad_bf16, grad_scale,
                         p0, p1, p2)
        else:
            ext.sgd_step_sched(self.mgr.master, self.mgr.grad, self.mom,
                               self.mgr.shadow, self.step_t, self.lr_table,
                               self.lr_out, self.lr, self.mu, self.wd,
                               self.nesterov, zero_grad, grad_bf16,
                               grad_scale, p0, p1, p2)
        self.mgr.stats_arena.zero_()
        self.mgr.refresh_rsck()

    def current_lr(self) -> float:
        """The learning rate the last update used.  Syncs — not for the hot
        loop."""
        if self.lr_out is None:
            return float(self.lr)
        return float(self.lr_out.cpu())

    def last_grad_norm(self) -> float:
        """Global L2 norm of the gradient the last update saw, before
        clipping.  Syncs — not for the hot loop."""
        if self.seg is None:
            raise RuntimeError("the gradient norm is only computed with "
                               "clip_grad_norm > 0 or lars")
        return self.seg.last_grad_norm()

    def set_step(self, n: int):
        """Position the schedule: the next ``step`` is update ``n`` (0-based).
        Without a schedule SGD keeps no counter and this does nothing."""
        if self.step_t is not None:
            self.step_t.fill_(float(n))

    def state_dict(self):
        state = {"kind": "horizon_sgd", "lr": self.lr, "momentum": self.mu,
                 "weight_decay": self.wd,
                 "mom": (self.mom.detach().cpu()
                         if self.mom is not None else None)}
        if self.step_t is not None:
            state["step_t"] = self.step_t.detach().cpu()
        return state

    def load_state_dict(self, state):
        if state.get("kind") != "horizon_sgd":
            raise ValueError("checkpoint optimizer state is not HorizonSGD")
        if (state.get("mom") is None) != (self.mom is None):
            raise ValueError("momentum buffer mismatch with checkpoint")
        self._live_stale = True  # loaded momentum: verify the table again
        with torch.no_grad():
            if self.mom is not None:
                self.mom.copy_(state["mom"].to(self.mom.device))
            # older checkpoints carry no counter: it stays where the caller
            # put it (set_step)
            if self.step_t is not None and state.get("step_t") is not None:
                self.step_t.copy_(state["step_t"].to(self.step_t.device))
