"""GPU side of the live-range optimizer step (``k_adam_step_live`` /
``k_sgd_step_live``, docs/KERNELS.md "Live-range step").

Op level: the live kernel, given an explicit table, against the full-range
kernel from the same state.  The update is one piece of code, so live
elements are compared bitwise; dead elements carry a NaN sentinel the live
kernel must neither read (the probe's sum would turn NaN) nor write.

Engine level: ResNet18 at 32x32, where 6 946 816 of 11.18 M elements are
layer4 taps that only meet padding, in deterministic mode so that the
gradient repeats bitwise and whole runs can be compared bitwise."""
import numpy as np
import pytest
import torch

from horizonml_amd.engine.flat import (FlatParamManager, HorizonAdam,
                                       HorizonSGD, build_live_chunks)
from horizonml_amd.engine.schedule import LRSchedule

pytestmark = pytest.mark.gpu

MU = 0.9
B1, B2, EPS = 0.9, 0.999, 1e-8
SENT32 = 0x7FC00ABC      # a quiet NaN with a recognisable payload
SENT16 = 0x7FC1
RESNET18_DEAD_AT_32 = 6946816


@pytest.fixture(scope="module")
def ext():
    from horizonml_amd import ops as _ops
    return _ops.extension()


def _dev():
    return torch.device("cuda", 0)


# ------------------------------------------------------------- op level ----
def _layout():
    """The flat buffer of the issue, in order.  Returns (numel, windows)."""
    windows, off = [], 0

    def vec(n):
        nonlocal off
        off += n

    def conv(K, Rf, Sf, C, r0, R, s0, S):
        nonlocal off
        windows.append((off, K, Rf, Sf, C, r0, R, s0, S))
        off += K * Rf * Sf * C

    vec(10)
    conv(8, 3, 3, 8, 1, 1, 1, 1)
    vec(8), vec(8)
    conv(8, 3, 3, 4, 1, 2, 1, 2)
    conv(4, 3, 3, 3, 1, 1, 1, 1)       # 3-element unaligned runs
    conv(4, 3, 3, 8, 1, 1, 0, 3)
    conv(8, 3, 3, 8, 0, 3, 0, 3)       # unclipped
    vec(7)
    conv(64, 3, 3, 64, 0, 3, 0, 3)     # fully live, several chunks
    return off, windows


@pytest.fixture(scope="module")
def table():
    numel, windows = _layout()
    chunks, n_dead = build_live_chunks(numel, windows)
    live = np.ones(numel, dtype=bool)
    for off, K, Rf, Sf, C, r0, R, s0, S in windows:
        w = live[off:off + K * Rf * Sf * C].reshape(K, Rf, Sf, C)
        keep = w[:, r0:r0 + R, s0:s0 + S].copy()
        w[:] = False
        w[:, r0:r0 + R, s0:s0 + S] = keep
    assert int((~live).sum()) == n_dead > 0
    assert len(chunks) > 9 and any(c[3] > 1 for c in chunks)
    return {"numel": numel,
            "chunks": torch.tensor(chunks, dtype=torch.int32, device=_dev()),
            "live": torch.from_numpy(live).to(_dev())}


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


class _State:
    """master, grad, first/second state, shadow, prev and the bf16 gradient;
    dead elements hold ``fill``: zeros for the full kernel, the sentinel for
    the live one."""

    def __init__(self, table, sentinel, adam, seed=5):
        g = torch.Generator().manual_seed(seed)
        n, self.live = table["numel"], table["live"]
        self.sentinel = sentinel
        self.master = self._mk(torch.randn(n, generator=g))
        self.grad = self._mk(torch.zeros(n))
        self.s1 = self._mk(torch.zeros(n))
        self.s2 = self._mk(torch.zeros(n)) if adam else None
        self.shadow = self._mk(self.master.to(torch.bfloat16))
        self.prev = self._mk(torch.randn(n, generator=g))
        self.gb = self._mk(torch.zeros(n, dtype=torch.bfloat16))
        self.step_t = torch.zeros(1, device=_dev())
        self.extra = torch.ones(37, device=_dev())
        self.lr_out = torch.full((1,), -1.0, device=_dev())
        self.sumsq = torch.zeros(1, device=_dev())
        self.out = torch.zeros(1, device=_dev())

    def _mk(self, t):
        t = t.to(_dev())
        dead = ~self.live
        if self.sentinel:
            _bits(t)[dead] = SENT32 if t.element_size() == 4 else SENT16
        else:
            t[dead] = 0
        return t

    def set_grad(self, g, bf16):
        self.grad[self.live] = g[self.live]
        if bf16:
            self.gb[self.live] = (g * 2).to(torch.bfloat16)[self.live]

    def flat(self):
        ts = [("master", self.master), ("grad", self.grad),
              ("state1", self.s1), ("shadow", self.shadow),
              ("prev", self.prev), ("grad_bf16", self.gb)]
        if self.s2 is not None:
            ts.append(("state2", self.s2))
        return ts


def _compare(new, ref, what):
    live, dead = new.live, ~new.live
    for (name, a), (_, b) in zip(new.flat(), ref.flat()):
        assert torch.equal(_bits(a)[live], _bits(b)[live]), \
            f"{what}: live {name} not bitwise the full kernel's"
        sent = SENT32 if a.element_size() == 4 else SENT16
        assert bool((_bits(a)[dead] == sent).all()), \
            f"{what}: a dead element of {name} was written"


ADAM_VARIANTS = ["plain", "keep_grad", "lr_table", "grad_bf16", "probe"]


@pytest.mark.parametrize("variant", ADAM_VARIANTS)
def test_adam_live_equals_full_kernel_on_live_elements(ext, table, variant):
    ref, new = _State(table, False, True), _State(table, True, True)
    zero_grad = variant != "keep_grad"
    bf16 = variant == "grad_bf16"
    sched = (LRSchedule("cosine", 0.05, 3, warmup_steps=1).table().to(_dev())
             if variant == "lr_table" else None)
    gen = torch.Generator().manual_seed(11)
    for k in range(4):                      # one step past the table's end
        g = torch.randn(table["numel"], generator=gen).to(_dev())
        outs = []
        for s in (ref, new):
            s.set_grad(g, bf16)
            s.extra.fill_(1.0)
            gb, gs = (s.gb, 0.5) if bf16 else (None, 1.0)
            pr = ((s.prev, s.sumsq, s.out) if variant == "probe"
                  else (None, None, None))
            if s is new:
                ext.adam_step_live(s.master, s.grad, s.s1, s.s2, s.shadow,
                                   s.step_t, sched,
                                   s.lr_out if sched is not None else None,
                                   0.01, B1, B2, EPS, zero_grad,
                                   table["chunks"], s.extra, gb, gs, *pr)
            elif sched is not None:
                ext.adam_step_sched(s.master, s.grad, s.s1, s.s2, s.shadow,
                                    s.step_t, sched, s.lr_out, 0.01, B1, B2,
                                    EPS, 0.0, False, zero_grad, s.extra, gb,
                                    gs, *pr)
            else:
                ext.adam_step(s.master, s.grad, s.s1, s.s2, s.shadow,
                              s.step_t, 0.01, B1, B2, EPS, 0.0, zero_grad,
                              s.extra, gb, gs, *pr)
            outs.append(float(s.out))
        _compare(new, ref, f"{variant} step {k}")
        assert torch.equal(new.step_t, ref.step_t)
        assert float(new.extra.abs().sum()) == 0.0
        assert torch.equal(new.lr_out, ref.lr_out)
        live_grad = new.grad[table["live"]]
        if zero_grad:
            assert float(live_grad.abs().sum()) == 0.0
        else:
            assert torch.equal(live_grad, g[table["live"]])
        if variant == "probe":
            # finite: no dead (NaN) element went into the sum.  Tolerance:
            # tests/test_ops_gpu.py::test_adam_fused_divergence_probe
            assert np.isfinite(outs[1]) and outs[0] > 0.0
            assert abs(outs[1] - outs[0]) / outs[0] < 1e-4
            assert float(new.sumsq) == 0.0
    assert sched is None or float(new.lr_out) == float(sched[-1])


SGD_VARIANTS = ["momentum", "no_momentum", "nesterov", "lr_table",
                "keep_grad", "grad_bf16", "probe"]


@pytest.mark.parametrize("variant", SGD_VARIANTS)
def test_sgd_live_equals_full_kernel_on_live_elements(ext, table, variant):
    ref, new = _State(table, False, False), _State(table, True, False)
    zero_grad = variant != "keep_grad"
    bf16 = variant == "grad_bf16"
    nesterov = variant == "nesterov"
    has_mom = variant != "no_momentum"
    sched = (LRSchedule("cosine", 0.05, 3, warmup_steps=1).table().to(_dev())
             if variant == "lr_table" else None)
    ex = nesterov or sched is not None
    gen = torch.Generator().manual_seed(12)
    for k in range(4):
        g = torch.randn(table["numel"], generator=gen).to(_dev())
        outs = []
        for s in (ref, new):
            s.set_grad(g, bf16)
            gb, gs = (s.gb, 0.5) if bf16 else (None, 1.0)
            pr = ((s.prev, s.sumsq, s.out) if variant == "probe"
                  else (None, None, None))
            mom = s.s1 if has_mom else None
            mu = MU if has_mom else 0.0
            st = s.step_t if sched is not None else None
            lo = s.lr_out if sched is not None else None
            if s is new:
                ext.sgd_step_live(s.master, s.grad, mom, s.shadow, st, sched,
                                  lo, 0.05, mu, nesterov, zero_grad,
                                  table["chunks"], gb, gs, *pr)
            elif ex:
                ext.sgd_step_sched(s.master, s.grad, mom, s.shadow, st,
                                   sched, lo, 0.05, mu, 0.0, nesterov,
                                   zero_grad, gb, gs, *pr)
            else:
                ext.sgd_step(s.master, s.grad, mom, s.shadow, 0.05, mu, 0.0,
                             zero_grad, gb, gs, *pr)
            outs.append(float(s.out))
        _compare(new, ref, f"{variant} step {k}")
        assert torch.equal(new.step_t, ref.step_t)
        assert torch.equal(new.lr_out, ref.lr_out)
        live_grad = new.grad[table["live"]]
        if zero_grad:
            assert float(live_grad.abs().sum()) == 0.0
        else:
            assert torch.equal(live_grad, g[table["live"]])
        if variant == "probe":
            assert np.isfinite(outs[1]) and outs[0] > 0.0
            assert abs(outs[1] - outs[0]) / outs[0] < 1e-4
            assert float(new.sumsq) == 0.0
    if not has_mom:   # the momentum slot was never touched
        assert bool((_bits(new.s1)[table["live"]] == 0).all())


def test_live_table_must_be_int32_nchunks_by_4(ext, table):
    s = _State(table, False, True)
    bad = [table["chunks"].to(torch.int64), table["chunks"][:, :3].contiguous(),
           table["chunks"].cpu(), table["chunks"][:0]]
    for t in bad:
        with pytest.raises(RuntimeError):
            ext.adam_step_live(s.master, s.grad, s.s1, s.s2, s.shadow,
                               s.step_t, None, None, 0.01, B1, B2, EPS, True,
                               t, None, None, 1.0, None, None, None)
    assert float(s.step_t) == 0.0


# --------------------------------------------------------- engine level ----
NAMES = ("master", "state1", "state2", "shadow", "grad")


def _batch(size, seed, bs=8):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(bs, 3, size, size, generator=g).to(_dev()).to(
        memory_format=torch.channels_last).to(torch.bfloat16)
    y = torch.randint(0, 10, (bs,), generator=g).to(_dev())
    return x, y


def _dead_element(model, mgr):
    """Offset of tap (0, 0) of the last 3x3x512 filter: dead at 32x32."""
    w = [p for p in model.parameters() if tuple(p.shape) == (512, 3, 3, 512)]
    return mgr.slices[id(w[-1])][0]


def _train(ext, sizes, skip, optname="adam", plant=False, wd_from=None,
           capture=False):
    """ResNet18, one step per entry of ``sizes`` on a fixed batch per size.
    Returns (final state clones, manager info, initial master, model)."""
    from horizonml_amd.models import resnet18
    from horizonml_amd.models._functional_gpu import cross_entropy
    was_det, was_skip = ext.deterministic_enabled(), ext.opt_skip_dead_enabled()
    ext.set_deterministic(True)
    ext.set_opt_skip_dead(skip)
    try:
        torch.manual_seed(0)
        model = resnet18(num_classes=10).to(_dev())
        model.train()
        mgr = FlatParamManager(model, _dev())
        opt = (HorizonAdam(mgr, lr=1e-3) if optname == "adam"
               else HorizonSGD(mgr, lr=0.05))
        master0 = mgr.master.clone()
        if plant:
            (opt.m if optname == "adam" else opt.mom)[
                _dead_element(model, mgr)] = 0.5
        batches = {s: _batch(s, 100 + s) for s in set(sizes)}

        def step(k):
            if wd_from is not None and k >= wd_from:
                opt.wd = 0.01
            x, y = batches[sizes[k]]
            cross_entropy(model(x), y).backward()
            opt.step()

        if capture:
            assert len(set(sizes)) == 1
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                step(0)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                step(1)
            for _ in sizes[1:]:
                graph.replay()
        else:
            for k in range(len(sizes)):
                step(k)
        torch.cuda.synchronize()
        s1 = opt.m if optname == "adam" else opt.mom
        s2 = opt.v if optname == "adam" else torch.zeros(1, device=_dev())
        state = [t.clone() for t in (mgr.master, s1, s2, mgr.shadow,
                                     mgr.grad)]
        return state, mgr.live_table_info(), master0, (model, mgr)
    finally:
        ext.set_deterministic(was_det)
        ext.set_opt_skip_dead(was_skip)


def _assert_bitwise(a, b, what):
    for x, y, nm in zip(a, b, NAMES):
        assert torch.equal(_bits(x), _bits(y)), f"{what}: {nm} differs"


@pytest.fixture(scope="module")
def full_adam_3(ext):
    """Three full-kernel Adam steps at 32x32: the reference several tests
    share.  Read only."""
    state, info, _, _ = _train(ext, [32, 32, 32], skip=False)
    assert info["state"] == "unbuilt"
    return state


def test_engine_adam_skip_equals_full_bitwise(ext, full_adam_3):
    state, info, master0, (model, mgr) = _train(ext, [32, 32, 32], skip=True)
    assert info["state"] == "live" and info["demoted"] == 0
    assert info["skipped"] == RESNET18_DEAD_AT_32
    _assert_bitwise(state, full_adam_3, "adam, 3 steps")
    d = _dead_element(model, mgr)
    assert state[0][d] == master0[d]              # identity on a dead tap
    assert not torch.equal(state[0], master0)     # and training happened


def test_engine_sgd_skip_equals_full_bitwise(ext):
    full, _, _, _ = _train(ext, [32, 32, 32], skip=False, optname="sgd")
    state, info, _, _ = _train(ext, [32, 32, 32], skip=True, optname="sgd")
    assert info["state"] == "live"
    assert info["skipped"] == RESNET18_DEAD_AT_32
    _assert_bitwise(state, full, "sgd, 3 steps")


def test_engine_captured_step_replayed_equals_eager(ext, full_adam_3):
    state, info, _, _ = _train(ext, [32, 32, 32], skip=True, capture=True)
    assert info["state"] == "live"
    assert info["skipped"] == RESNET18_DEAD_AT_32
    _assert_bitwise(state, full_adam_3, "1 eager + 2 replays")


def test_engine_planted_moment_keeps_the_tensor_live(ext):
    full, _, _, _ = _train(ext, [32, 32], skip=False, plant=True)
    state, info, _, _ = _train(ext, [32, 32], skip=True, plant=True)
    assert info["state"] == "live" and info["demoted"] == 1
    assert info["skipped"] == RESNET18_DEAD_AT_32 - 512 * 8 * 512
    _assert_bitwise(state, full, "planted m")


def test_engine_weight_decay_runs_the_full_kernel(ext):
    full, _, _, _ = _train(ext, [32, 32, 32], skip=False, wd_from=1)
    state, info, master0, (model, mgr) = _train(ext, [32, 32, 32], skip=True,
                                                wd_from=1)
    assert info["state"] == "live"       # built by the first, decay-free step
    _assert_bitwise(state, full, "wd set after one step")
    d = _dead_element(model, mgr)
    assert master0[d] != 0 and state[0][d] != master0[d]   # dead taps decay


def test_engine_resolution_change_rebuilds_the_union(ext):
    sizes = [32, 32, 64, 64]
    full, _, _, _ = _train(ext, sizes, skip=False)
    v0 = ext.tap_window_version()
    state, info, _, (model, mgr) = _train(ext, sizes, skip=True)
    assert ext.tap_window_version() > v0
    assert info["version"] == ext.tap_window_version()
    # at 64x64 every layer4 tap meets a pixel: the union has no dead element
    assert info["state"] == "none" and info["skipped"] == 0
    for w in mgr.live_windows():
        assert (w[5], w[6], w[7], w[8]) == (0, w[2], 0, w[3])
    _assert_bitwise(state, full, "2 steps at 32, 2 at 64")


def test_model_without_dead_taps_reports_none(ext):
    _, info, _, _ = _train(ext, [64], skip=True)
    assert info["state"] == "none"
    assert info["skipped"] == 0 and info["nchunks"] == 0
