"""GPU side of the segmented fused step: per-segment weight decay, global-norm
clipping and the LARS trust ratio (``k_seg_sumsq_partial`` / ``k_seg_finalize``
/ ``k_sgd_step_seg`` / ``k_adam_step_seg``).

The synthetic flat buffer has segment sizes 1, 3, 64, 4096, 4097, 10, 8193, 7:
single-element, sub-vector, exactly one chunk, chunk + 1, multi-chunk, and
unaligned starts after the odd sizes.  The five small ones play the 1-D
parameters (``decay = adapt = 0``).

References: the existing ``*_step_sched`` ops (bitwise, uniform table), torch
optimizers with two param groups, and ``engine.lars.LARS`` on float64 copies
(the contract in plain torch).  Measured errors: docs/VALIDATION_LOG.md.
"""
import functools

import numpy as np
import pytest
import torch

from horizonml_amd.engine.lars import LARS
from horizonml_amd.engine.schedule import LRSchedule

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 64, 4096, 4097, 10, 8193, 7]
ONE_D = [n in (1, 3, 64, 10, 7) for n in SIZES]
BOUNDS = np.concatenate([[0], np.cumsum(SIZES)]).tolist()
N_EL = BOUNDS[-1]
MU, WD, ETA = 0.9, 5e-4, 1e-3
B1, B2, EPS = 0.9, 0.999, 1e-8
STEPS = 3


@pytest.fixture(scope="module")
def ext():
    from horizonml_amd import ops as _ops
    return _ops.extension()


def _dev():
    return torch.device("cuda", 0)


def rel(a, b):  # the file-local rel() of tests/test_ops_gpu.py
    a = a.float().cpu()
    b = b.float().cpu()
    d = (a - b).norm()
    return (d / b.norm().clamp_min(1e-12)).item()


def _table(no_decay=True):
    from horizonml_amd.engine.flat import SegmentTable
    return SegmentTable(SIZES, [not (no_decay and d) for d in ONE_D],
                        [not d for d in ONE_D], _dev())


@functools.lru_cache(maxsize=None)
def _inputs(seed=0, dyadic=False):
    """(master0, [grad per step]) on the CPU, float32; shared, never
    written."""
    g = torch.Generator().manual_seed(seed)
    master0 = torch.randn(N_EL, generator=g)
    grads = [torch.randn(N_EL, generator=g) for _ in range(STEPS + 1)]
    if dyadic:  # see test_scheduled_adam_equals_existing_op_bitwise
        grads = [(x * 8).round() / 8 for x in grads]
    return master0, grads


class _State:
    def __init__(self, master0):
        dev = _dev()
        self.master = master0.to(dev).clone()
        self.grad = torch.zeros_like(self.master)
        self.mom = torch.zeros_like(self.master)
        self.m = torch.zeros_like(self.master)
        self.v = torch.zeros_like(self.master)
        self.shadow = torch.zeros_like(self.master, dtype=torch.bfloat16)
        self.step_t = torch.zeros(1, device=dev)
        self.extra = torch.ones(37, device=dev)

    def tensors(self):
        return (self.master, self.grad, self.mom, self.m, self.v,
                self.shadow, self.step_t, self.extra)

    NAMES = ("master", "grad", "mom", "m", "v", "shadow", "step_t", "extra")


def _assert_same(a, b):
    for x, y, nm in zip(a.tensors(), b.tensors(), _State.NAMES):
        assert torch.equal(x, y), f"{nm} not bitwise equal"


class _Seg:
    """Table + the buffers of the norm reduction, as ``flat._SegState``
    keeps them."""

    def __init__(self, table, wd, max_norm=0.0, lars=False, eta=ETA):
        self.t, self.wd, self.max_norm = table, wd, max_norm
        self.lars, self.eta = lars, eta
        dev = _dev()
        self.mul = table.static_mul(wd)
        self.partials = torch.full((table.nchunks, 2), 7.0, device=dev)
        self.norms = torch.full((table.nseg, 2), 7.0, device=dev)
        self.out = torch.full((2,), 7.0, device=dev)
        self.dynamic = max_norm > 0 or lars

    def reduce(self, ext, st, gb=None, gs=1.0):
        if self.dynamic:
            ext.seg_norms(st.master, st.grad, self.t.chunks, self.t.seg_meta,
                          self.partials, self.norms, self.mul, self.out,
                          self.wd, self.max_norm, self.lars, self.eta, gb, gs)

    def sgd(self, ext, st, lr, nesterov, table=None, lr_out=None, gb=None,
            gs=1.0, probe=(None, None, None), zero_grad=True):
        self.reduce(ext, st, gb, gs)
        ext.sgd_step_seg(st.master, st.grad, st.mom, st.shadow,
                         st.step_t if table is not None else None, table,
                         lr_out, lr, MU, nesterov, zero_grad, self.t.chunks,
                         self.mul, gb, gs, *probe)

    def adam(self, ext, st, lr, decoupled, table=None, lr_out=None, gb=None,
             gs=1.0, probe=(None, None, None), zero_grad=True):
        self.reduce(ext, st, gb, gs)
        ext.adam_step_seg(st.master, st.grad, st.m, st.v, st.shadow,
                          st.step_t, table, lr_out, lr, B1, B2, EPS,
                          decoupled, zero_grad, self.t.chunks, self.mul,
                          st.extra, gb, gs, *probe)


def _seg_params(flat, dtype):
    """Per-segment leaf tensors of a flat CPU vector: 1-D for the 1-D-like
    segments, [1, n] for the rest (so ``ndim`` carries ``adapt``)."""
    ps = []
    for s, n in enumerate(SIZES):
        x = flat[BOUNDS[s]:BOUNDS[s + 1]].to(dtype).clone()
        ps.append((x if ONE_D[s] else x.view(1, n)).requires_grad_(True))
    return ps


def _groups(ps, wd, no_decay=True):
    return [{"params": [p for p, d in zip(ps, ONE_D) if not (no_decay and d)],
             "weight_decay": wd},
            {"params": [p for p, d in zip(ps, ONE_D) if no_decay and d],
             "weight_decay": 0.0}]


def _set_grads(ps, g, dtype):
    for s, p in enumerate(ps):
        p.grad = g[BOUNDS[s]:BOUNDS[s + 1]].to(dtype).view(p.shape).clone()


def _flat(ps):
    return torch.cat([p.detach().flatten() for p in ps])


# ------------------------------------------- 1. uniform table == existing op --
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("flag", [False, True])   # Nesterov / decoupled
@pytest.mark.parametrize("sched", [False, True])
@pytest.mark.parametrize("which", ["sgd", "adam"])
def test_uniform_table_equals_existing_op_bitwise(ext, which, sched, flag,
                                                  bf16):
    master0, grads = _inputs(1)
    ref, new = _State(master0), _State(master0)
    seg = _Seg(_table(no_decay=False), WD)
    dtab = (LRSchedule("cosine", 0.1, 5, warmup_steps=2).table().to(_dev())
            if sched else None)
    lo_r = torch.full((1,), -1.0, device=_dev())
    lo_n = torch.full((1,), -1.0, device=_dev())
    for g in grads[:STEPS]:
        g = g.to(_dev())
        ref.grad.copy_(g), new.grad.copy_(g)
        ref.extra.fill_(1.0), new.extra.fill_(1.0)
        gb, gs = ((g * 2).to(torch.bfloat16), 0.5) if bf16 else (None, 1.0)
        if which == "sgd":
            ext.sgd_step_sched(ref.master, ref.grad, ref.mom, ref.shadow,
                               ref.step_t if sched else None, dtab, lo_r,
                               0.05, MU, WD, flag, True, gb, gs)
            seg.sgd(ext, new, 0.05, flag, dtab, lo_n, gb, gs)
        else:
            ext.adam_step_sched(ref.master, ref.grad, ref.m, ref.v,
                                ref.shadow, ref.step_t, dtab, lo_r, 0.05, B1,
                                B2, EPS, WD, flag, True, ref.extra, gb, gs)
            seg.adam(ext, new, 0.05, flag, dtab, lo_n, gb, gs)
        _assert_same(new, ref)
        assert torch.equal(lo_n, lo_r)
    assert float(new.grad.abs().sum()) == 0.0
    if which == "adam":
        assert float(new.extra.abs().sum()) == 0.0


@pytest.mark.parametrize("which", ["sgd", "adam"])
def test_uniform_table_probe_bitwise(ext, which):
    """Probe on, dyadic gradients (multiples of 1/8): every (g - prev)^2 and
    every partial sum is exact in f32, so the chunk-partitioned sum equals the
    grid-stride one whatever the order of the atomics."""
    master0, grads = _inputs(2, dyadic=True)
    ref, new = _State(master0), _State(master0)
    seg = _Seg(_table(no_decay=False), WD)
    prev0 = grads[STEPS].to(_dev())
    pr, pn = [(prev0.clone(), torch.zeros(1, device=_dev()),
               torch.zeros(1, device=_dev())) for _ in range(2)]
    for g in grads[:STEPS]:
        g = g.to(_dev())
        ref.grad.copy_(g), new.grad.copy_(g)
        if which == "sgd":
            ext.sgd_step_sched(ref.master, ref.grad, ref.mom, ref.shadow,
                               None, None, None, 0.05, MU, WD, True, True,
                               None, 1.0, *pr)
            seg.sgd(ext, new, 0.05, True, probe=pn)
        else:
            ext.adam_step_sched(ref.master, ref.grad, ref.m, ref.v,
                                ref.shadow, ref.step_t, None, None, 0.05, B1,
                                B2, EPS, WD, True, True, ref.extra, None,
                                1.0, *pr)
            seg.adam(ext, new, 0.05, True, probe=pn)
        _assert_same(new, ref)
        assert torch.equal(pn[0], pr[0]) and torch.equal(pn[0], g)   # prev
        assert float(pn[1]) == 0.0                              # sumsq reset
        assert float(pn[2]) > 0.0 and torch.equal(pn[2], pr[2])     # output


# ------------------------------------------------------------- 2. no-decay --
@pytest.mark.parametrize("which", ["sgd", "adamw"])
def test_no_decay_matches_torch_param_groups(ext, which):
    master0, grads = _inputs(3)
    ps = _seg_params(master0, torch.float32)
    if which == "sgd":
        opt = torch.optim.SGD(_groups(ps, WD), lr=0.1, momentum=MU,
                              nesterov=True)
    else:
        opt = torch.optim.AdamW(_groups(ps, 1e-2), lr=1e-3)
    st = _State(master0)
    seg = _Seg(_table(), WD if which == "sgd" else 1e-2)
    for g in grads[:STEPS]:
        _set_grads(ps, g, torch.float32)
        opt.step()
        st.grad.copy_(g.to(_dev()))
        if which == "sgd":
            seg.sgd(ext, st, 0.1, True)
        else:
            seg.adam(ext, st, 1e-3, True)
    r = rel(st.master, _flat(ps))
    print(f"no_decay {which} rel={r:.3e}")
    assert r < 1e-5
    # the decay really differs between the two groups
    uni = _State(master0)
    useg = _Seg(_table(no_decay=False), WD if which == "sgd" else 1e-2)
    for g in grads[:STEPS]:
        uni.grad.copy_(g.to(_dev()))
        (useg.sgd(ext, uni, 0.1, True) if which == "sgd"
         else useg.adam(ext, uni, 1e-3, True))
    for s in range(len(SIZES)):
        same = torch.equal(uni.master[BOUNDS[s]:BOUNDS[s + 1]],
                           st.master[BOUNDS[s]:BOUNDS[s + 1]])
        assert same == (not ONE_D[s]), s


@pytest.mark.parametrize("which", ["sgd", "adam", "adamw"])
def test_no_decay_segments_untouched_by_zero_gradient(ext, which):
    master0, _ = _inputs(3)
    st = _State(master0)
    seg = _Seg(_table(), 0.1)
    if which == "sgd":
        seg.sgd(ext, st, 0.1, False)
    else:
        seg.adam(ext, st, 0.1, which == "adamw")
    m0 = master0.to(_dev())
    for s in range(len(SIZES)):
        same = torch.equal(st.master[BOUNDS[s]:BOUNDS[s + 1]],
                           m0[BOUNDS[s]:BOUNDS[s + 1]])
        assert same == ONE_D[s], (s, SIZES[s])
    assert torch.isfinite(st.master).all()


# ----------------------------------------------------------------- 3. norms --
def _norms64(w, g, wd, max_norm, lars, no_decay=True):
    """The contract in float64 on flat CPU vectors: N, c, q_s."""
    w, g = w.double(), g.double()
    G = [float((g[BOUNDS[s]:BOUNDS[s + 1]] ** 2).sum())
         for s in range(len(SIZES))]
    W = [float((w[BOUNDS[s]:BOUNDS[s + 1]] ** 2).sum())
         for s in range(len(SIZES))]
    N = float(np.sqrt(sum(G)))
    c = min(1.0, max_norm / (N + 1e-6)) if max_norm > 0 else 1.0
    q = []
    for s in range(len(SIZES)):
        wd_s = 0.0 if (no_decay and ONE_D[s]) else wd
        gn, wn = c * np.sqrt(G[s]), np.sqrt(W[s])
        ok = lars and not ONE_D[s] and wn > 0 and gn > 0
        q.append(ETA * wn / (gn + wd_s * wn + 1e-8) if ok else 1.0)
    return N, c, q, G, W


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("max_norm", [0.0, 40.0])
def test_norms_against_float64(ext, max_norm, bf16):
    master0, grads = _inputs(4)
    st = _State(master0)
    st.grad.copy_(grads[0].to(_dev()))
    gb, gs, g_eff = None, 1.0, grads[0]
    if bf16:  # the norm is that of b2f(gsrc)*gscale, not of the local grad
        gb = (grads[1] * 4).to(torch.bfloat16).to(_dev())
        gs = 0.5
        g_eff = gb.cpu().double() * 0.5
    seg = _Seg(_table(), WD, max_norm, lars=True)
    seg.reduce(ext, st, gb, gs)
    N, c, q, G, W = _norms64(master0, g_eff, WD, max_norm, True)
    out = seg.out.cpu().double()
    e_n = abs(out[0].item() - N) / N
    e_c = abs(out[1].item() - c) / c
    mul, nrm = seg.mul.cpu().double(), seg.norms.cpu().double()
    e_q = max(abs(mul[s, 0].item() / out[1].item() - q[s]) / q[s]
              for s in range(len(SIZES)))
    e_g = max(abs(nrm[s, 0].item() - G[s]) / G[s] for s in range(len(SIZES)))
    e_w = max(abs(nrm[s, 1].item() - W[s]) / W[s] for s in range(len(SIZES)))
    print(f"norms max_norm={max_norm} bf16={bf16}: N {e_n:.3e} c {e_c:.3e} "
          f"q {e_q:.3e} G_s {e_g:.3e} W_s {e_w:.3e}")
    assert (max_norm > 0) == (c < 1.0)
    assert e_n < 1e-5 and e_c < 1e-5 and e_q < 1e-5
    assert e_g < 1e-5 and e_w < 1e-5
    for s in range(len(SIZES)):     # wmul = q * wd_s, and q = 1 on 1-D
        wd_s = 0.0 if ONE_D[s] else WD
        assert abs(mul[s, 1].item() - q[s] * wd_s) <= 1e-5 * q[s] * wd_s
        if ONE_D[s]:
            assert mul[s, 0].item() == out[1].item()
    if bf16:  # and differs from the local gradient's norm
        N_local = float(grads[0].double().norm())
        assert abs(out[0].item() - N_local) / N_local > 1e-3


# ------------------------------------------------------------------ 4. clip --
@pytest.mark.parametrize("which", ["sgd", "adam"])
def test_clip_matches_clip_grad_norm(ext, which):
    """max_norm once at half the smallest and once at twice the largest of
    the three steps' norms.  Below: against clip_grad_norm_ + torch in
    float64.  Above: c = 1, bitwise the unclipped segmented step."""
    master0, grads = _inputs(5)
    norms = [float(g.double().norm()) for g in grads[:STEPS]]
    lo, hi = 0.5 * min(norms), 2.0 * max(norms)
    ps = _seg_params(master0, torch.float64)
    opt = (torch.optim.SGD(_groups(ps, WD), lr=0.1, momentum=MU)
           if which == "sgd" else torch.optim.Adam(_groups(ps, WD), lr=1e-3))
    clipped, above, plain = (_State(master0) for _ in range(3))
    s_lo, s_hi = _Seg(_table(), WD, lo), _Seg(_table(), WD, hi)
    s_off = _Seg(_table(), WD)
    for k, g in enumerate(grads[:STEPS]):
        _set_grads(ps, g, torch.float64)
        torch.nn.utils.clip_grad_norm_(ps, lo)
        opt.step()
        for st in (clipped, above, plain):
            st.grad.copy_(g.to(_dev()))
        for seg, st in ((s_lo, clipped), (s_hi, above), (s_off, plain)):
            (seg.sgd(ext, st, 0.1, False) if which == "sgd"
             else seg.adam(ext, st, 1e-3, False))
        assert abs(s_lo.out[0].item() - norms[k]) < 1e-5 * norms[k]
        assert s_hi.out[1].item() == 1.0
    _assert_same(above, plain)
    r = rel(clipped.master, _flat(ps))
    rm = rel(clipped.mom if which == "sgd" else clipped.m,
             torch.cat([(opt.state[p]["momentum_buffer"] if which == "sgd"
                         else opt.state[p]["exp_avg"]).flatten()
                        for p in ps]))
    print(f"clip {which}: master rel={r:.3e} momentum rel={rm:.3e}")
    assert r < 1e-5 and rm < 1e-5


def test_clipped_update_has_norm_max_norm(ext):
    """One plain SGD step (no momentum, no decay): (w0 - w1)/lr is the
    gradient the update applied, and its norm must be max_norm.  Bound: each
    w1 is rounded once, an error of at most 2^-24*|w| per element, so the
    implied gradient's norm is off by at most 2^-24*|w|_2/lr = 7.7e-5 here
    (|w|_2 ~ 128, lr = 0.1), 2.4e-6 of max_norm = 32; c and N add a few
    2^-24 relative.  1e-5 leaves a factor of 3."""
    master0, grads = _inputs(5)
    st = _State(master0)
    st.grad.copy_(grads[0].to(_dev()))
    max_norm, lr = 32.0, 0.1
    assert float(grads[0].double().norm()) > 2 * max_norm
    seg = _Seg(_table(), 0.0, max_norm)
    ext.seg_norms(st.master, st.grad, seg.t.chunks, seg.t.seg_meta,
                  seg.partials, seg.norms, seg.mul, seg.out, 0.0, max_norm,
                  False, ETA)
    ext.sgd_step_seg(st.master, st.grad, None, None, None, None, None, lr,
                     0.0, False, False, seg.t.chunks, seg.mul)
    implied = (master0.double() - st.master.cpu().double()) / lr
    e = abs(float(implied.norm()) - max_norm) / max_norm
    print(f"clipped update: implied norm rel err {e:.3e}")
    assert e < 1e-5
    cos = float((implied * grads[0].double()).sum()
                / (implied.norm() * grads[0].double().norm()))
    assert cos > 1 - 1e-6       # and it is the gradient, scaled


# ------------------------------------------------------------------ 5. LARS --
@functools.lru_cache(maxsize=None)
def _lars_ref(nesterov, wd, max_norm, dtype, degenerate=False):
    """STEPS steps of ``engine.lars.LARS`` on CPU copies: (master, mom)."""
    master0, grads = _lars_inputs(degenerate)
    ps = _seg_params(master0, dtype)
    opt = LARS(_groups(ps, wd), lr=0.1, momentum=MU, nesterov=nesterov,
               eta=ETA, max_norm=max_norm)
    for g in grads[:STEPS]:
        _set_grads(ps, g, dtype)
        opt.step()
    return _flat(ps), torch.cat([opt.state[p]["momentum_buffer"].flatten()
                                 for p in ps])


@functools.lru_cache(maxsize=None)
def _lars_inputs(degenerate):
    master0, grads = _inputs(6)
    if degenerate:  # adapt segments: 3 has w = 0, 4 has g = 0
        master0 = master0.clone()
        master0[BOUNDS[3]:BOUNDS[4]] = 0.0
        grads = [g.clone() for g in grads]
        for g in grads:
            g[BOUNDS[4]:BOUNDS[5]] = 0.0
    return master0, grads


def _lars_gpu(ext, nesterov, wd, max_norm, degenerate=False):
    master0, grads = _lars_inputs(degenerate)
    st = _State(master0)
    seg = _Seg(_table(), wd, max_norm, lars=True)
    muls = []
    for g in grads[:STEPS]:
        st.grad.copy_(g.to(_dev()))
        seg.sgd(ext, st, 0.1, nesterov)
        muls.append((seg.mul.clone(), seg.out.clone()))
    return st, muls


@pytest.mark.parametrize("max_norm", [0.0, 50.0])
@pytest.mark.parametrize("wd", [0.0, WD])
@pytest.mark.parametrize("nesterov", [False, True])
def test_lars_matches_float64_reference(ext, nesterov, wd, max_norm):
    st, _ = _lars_gpu(ext, nesterov, wd, max_norm)
    w64, u64 = _lars_ref(nesterov, wd, max_norm, torch.float64)
    w32, u32 = _lars_ref(nesterov, wd, max_norm, torch.float32)
    r_w, r_u = rel(st.master, w64), rel(st.mom, u64)
    t_w = ((w32.double() - w64).norm() / w64.norm()).item()
    t_u = ((u32.double() - u64).norm() / u64.norm()).item()
    print(f"lars nesterov={nesterov} wd={wd} max_norm={max_norm}: kernel "
          f"master {r_w:.3e} mom {r_u:.3e} | f32 torch master {t_w:.3e} "
          f"mom {t_u:.3e}")
    assert r_w < 1e-5 and r_u < 1e-5
    # the trust ratio really acted: far from plain SGD on the same inputs
    master0, grads = _lars_inputs(False)
    plain = _State(master0)
    pseg = _Seg(_table(), wd, max_norm)
    for g in grads[:STEPS]:
        plain.grad.copy_(g.to(_dev()))
        pseg.sgd(ext, plain, 0.1, nesterov)
    assert rel(plain.master, w64) > 1e-2


def test_lars_degenerate_segments_take_q_one(ext):
    st, muls = _lars_gpu(ext, True, WD, 50.0, degenerate=True)
    mul, out = muls[0]
    c = out[1].item()
    assert 0 < c < 1
    # step 0: segment 3 has w = 0, segment 4 has g = 0 -> q = 1
    assert mul[3, 0].item() == c and mul[3, 1].item() == np.float32(WD)
    assert mul[4, 0].item() == c and mul[4, 1].item() == np.float32(WD)
    assert mul[6, 0].item() != c            # a live adapt segment
    assert torch.isfinite(st.master).all() and torch.isfinite(st.mom).all()
    for m, _ in muls:
        assert torch.isfinite(m).all()
    w64, u64 = _lars_ref(True, WD, 50.0, torch.float64, True)
    assert rel(st.master, w64) < 1e-5 and rel(st.mom, u64) < 1e-5


# ---------------------------------------------------------- 6. graph replay --
def test_graph_replay_equals_eager_bitwise(ext):
    """partials -> finalize -> step in one captured graph, replayed with a new
    gradient each time.  Accumulating partials or seg_mul, or norms baked in
    at capture, would show from the second replay on."""
    R = 4
    master0, grads = _inputs(7)
    grads = [grads[k % len(grads)] * (1 + k) for k in range(R)]
    ref, new = _State(master0), _State(master0)
    s_ref = _Seg(_table(), WD, 50.0, lars=True)
    s_new = _Seg(_table(), WD, 50.0, lars=True)
    new.grad.copy_(grads[0].to(_dev()))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s_new.sgd(ext, new, 0.1, True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for t, f in zip(new.tensors(), _State(master0).tensors()):
        t.copy_(f)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s_new.sgd(ext, new, 0.1, True)
    assert torch.equal(new.master, master0.to(_dev()))
    seen = []
    for k in range(R):
        new.grad.copy_(grads[k].to(_dev()))   # static buffer, new contents
        graph.replay()
        seen.append(s_new.out.clone())
        ref.grad.copy_(grads[k].to(_dev()))
        s_ref.sgd(ext, ref, 0.1, True)
        assert torch.equal(s_new.out, s_ref.out), k
        assert torch.equal(s_new.mul, s_ref.mul), k
    torch.cuda.synchronize()
    _assert_same(new, ref)
    assert len({x[0].item() for x in seen}) == R    # the norm really moved


# ---------------------------------------------------------- 7. reproducible --
def test_two_runs_are_bitwise_equal(ext):
    a, ma = _lars_gpu(ext, True, WD, 50.0)
    b, mb = _lars_gpu(ext, True, WD, 50.0)
    _assert_same(a, b)
    for (m1, o1), (m2, o2) in zip(ma, mb):
        assert torch.equal(m1, m2) and torch.equal(o1, o2)


def test_seg_argument_checks(ext):
    master0, _ = _inputs(0)
    st = _State(master0)
    seg = _Seg(_table(), WD, 1.0, lars=True)

    def norms(chunks=seg.t.chunks, meta=seg.t.seg_meta, part=seg.partials,
              mul=seg.mul, out=seg.out, master=st.master):
        ext.seg_norms(master, st.grad, chunks, meta, part, seg.norms, mul,
                      out, WD, 1.0, True, ETA)

    for bad in (dict(chunks=seg.t.chunks.long()),
                dict(chunks=seg.t.chunks.cpu()),
                dict(meta=seg.t.seg_meta[:-1]),
                dict(part=seg.partials[:-1]),
                dict(mul=seg.mul.double()),
                dict(out=torch.zeros(1, device=_dev())),
                dict(master=st.master[1:])):
        with pytest.raises(RuntimeError):
            norms(**bad)
    with pytest.raises(RuntimeError):
        ext.sgd_step_seg(st.master, st.grad, st.mom, st.shadow, None, None,
                         None, 0.1, MU, False, True, seg.t.chunks.long(),
                         seg.mul)
    torch.cuda.synchronize()
    assert float(seg.out[0]) == 7.0             # nothing was launched
    assert torch.equal(st.master, master0.to(_dev()))


# --------------------------------------------------- 8. through the manager --
def test_options_drive_the_flat_manager(ext):
    from horizonml_amd.engine.flat import (FlatParamManager, HorizonAdam,
                                           HorizonSGD)
    from horizonml_amd.models import resnet18
    from horizonml_amd.models._functional_gpu import cross_entropy
    torch.manual_seed(0)
    dev = _dev()
    defer_was = ext.wgrad_defer_enabled()
    try:
        model = resnet18(num_classes=10).to(dev)
        mgr = FlatParamManager(model, dev)
        for opt in (HorizonSGD(mgr), HorizonAdam(mgr)):
            assert opt.seg is None          # defaults allocate nothing
            with pytest.raises(RuntimeError):
                opt.last_grad_norm()
        assert mgr._seg_tables == {}
        opt = HorizonSGD(mgr, lr=0.05, weight_decay=5e-4, nesterov=True,
                         lars=True, clip_grad_norm=1.0, no_decay_1d=True)
        t = opt.seg.table
        assert t.bounds[0] == 0 and t.bounds[-1] == mgr.numel
        assert t.sizes == [p.numel() for p in mgr.params]
        ch = t.chunks.cpu().numpy()
        assert ch[0, 1] == 0 and (ch[:, 2] >= 1).all()
        assert (ch[:, 2] <= 4096).all()
        assert (ch[1:, 1] == ch[:-1, 1] + ch[:-1, 2]).all()   # exactly once
        assert ch[-1, 1] + ch[-1, 2] == mgr.numel
        meta = t.seg_meta.cpu().numpy()
        for s in range(t.nseg):
            c0, c1 = meta[s, 0], meta[s, 1]
            assert (ch[c0:c1, 0] == s).all()
            assert ch[c0, 1] == t.bounds[s]
            assert ch[c1 - 1, 1] + ch[c1 - 1, 2] == t.bounds[s + 1]
        one_d = sum(p.ndim <= 1 for p in model.parameters())
        assert one_d > 0
        assert sum(not d for d in t.decay) == one_d
        assert sum(not a for a in t.adapt) == one_d
        x = torch.randn(8, 3, 32, 32, device=dev).to(
            memory_format=torch.channels_last).to(torch.bfloat16)
        y = torch.randint(0, 10, (8,), device=dev)
        start = mgr.master.clone()
        for _ in range(2):
            loss = cross_entropy(model(x), y)
            loss.backward()
            opt.step()
            assert np.isfinite(loss.item())
            assert opt.last_grad_norm() > 0
        assert torch.isfinite(mgr.master).all()
        assert not torch.equal(mgr.master, start)
        assert torch.equal(mgr.shadow, mgr.master.to(torch.bfloat16))
        assert float(mgr.grad.abs().sum()) == 0.0
        assert ext.wgrad_pending() == 0
        adam = HorizonAdam(mgr, clip_grad_norm=1.0, no_decay_1d=True,
                           weight_decay=1e-2, decoupled_wd=True)
        cross_entropy(model(x), y).backward()
        adam.step()
        assert adam.last_grad_norm() > 0 and torch.isfinite(mgr.master).all()
        assert float(mgr.stats_arena.abs().sum()) == 0.0
        assert ext.wgrad_pending() == 0
    finally:
        ext.set_wgrad_defer(defer_was)


# ---------------------------------------------------- 9. engine end to end --
_COLS = ["epoch", "loss", "accuracy", "epoch_time", "avg_step_time",
         "compute_time", "comm_time", "idle_time", "avg_cpu", "avg_memory",
         "grad_divergence", "gpu_memory_mb", "gpu_util", "worker",
         "total_training_time"]


def _run(tmp_path, tag, **kw):
    from data_parallel_train import run_data_parallel
    df = run_data_parallel(1, 2, 256, str(tmp_path / tag), batch_size=64,
                           synthetic=True, engine="flat", **kw)
    assert df is not None and len(df) == 2
    assert np.isfinite(df["loss"].to_numpy()).all()
    assert sorted(df.columns) == sorted(_COLS)   # the CSV schema is fixed
    return df


@pytest.mark.timeout(300)
def test_dp_flat_lars_end_to_end(tmp_path):
    _run(tmp_path, "lars", optimizer_name="sgd", lr=0.1, nesterov=True,
         lr_schedule="cosine", warmup_epochs=1, weight_decay=5e-4,
         lars=True, clip_grad_norm=5.0, no_decay_1d=True)


@pytest.mark.timeout(300)
def test_dp_flat_adamw_clip_end_to_end(tmp_path):
    _run(tmp_path, "adamw", optimizer_name="adam", lr=1e-3,
         decoupled_wd=True, weight_decay=1e-2, clip_grad_norm=1.0,
         no_decay_1d=True)
