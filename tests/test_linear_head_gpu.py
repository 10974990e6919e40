"""Classifier tail: one-launch linear backward, cross-entropy that stores its
loss.  (The forward kernel is unchanged: a grouped reduction measured slower
and was not kept, docs/STATUS.md.)

Each new kernel sits behind a runtime switch whose off state launches the
former kernels, so the former kernels are the bitwise reference wherever the
arithmetic per output is unchanged (dx, loss, dlogits).  dW and db of
the fused backward sum the batch in another order; they are held to the f32
summation bound against float64.

The bound.  With u = 2^-24, a sum of B terms in any order of f32 additions is
within B*u*S of the exact sum, S the sum of the terms' magnitudes, as long as
the terms themselves are exact: every term then passes through at most B - 1
roundings, and the accumulating add into an initial value v0 costs one more,
u*|v0 + sum| <= ulp(v0) + u*S.  A rounded product would add one rounding per
term on top, which at B = 1 (and only there) no kernel, the former ones
included, can fit into 1*u*S.  So the bound test draws dy from the f32 numbers
that bf16 holds exactly: x is bf16, the products dy*x then have 16 significant
bits and are exact in f32, and the bound holds as derived.  The bitwise tests
draw dy from all of f32.
"""
import functools
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _C():
    from horizonml_amd import ops
    return ops.extension()


class _switch:
    """Set one of the extension's switches for a block, then restore it."""

    def __init__(self, name, on):
        self.name, self.on = name, on

    def __enter__(self):
        C = _C()
        getter = {"deterministic": "deterministic_enabled"}.get(
            self.name, self.name + "_enabled")
        self.was = getattr(C, getter)()
        getattr(C, "set_" + self.name)(self.on)

    def __exit__(self, *exc):
        getattr(_C(), "set_" + self.name)(self.was)


def _ulp(t):
    """Spacing of f32 at |t| (t float64 holding f32 values)."""
    m, e = torch.frexp(t.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(t), e - 24)


# ------------------------------------------------------------- backward -----
BWD_B = [1, 3, 64, 128]        # one row; row-lanes not filled; flagship; limit
BWD_IN = [8, 24, 512, 1032]    # one vec8; partial slice; flagship; partial last
BWD_OUT = [1, 10, 16]
# (accum, with_db, with_dx)
VARIANTS = list(itertools.product([0, 1], [True, False], [True, False]))


@functools.lru_cache(maxsize=None)
def _bwd_inputs(B, In, Out):
    g = torch.Generator().manual_seed(B * 100003 + In * 101 + Out)
    x = torch.randn(B, In, generator=g).bfloat16()
    w = (torch.randn(Out, In, generator=g) * 0.1).bfloat16()
    dy = torch.randn(B, Out, generator=g) * 0.3
    dyq = dy.bfloat16().float()          # exact in bf16: exact products
    pre_w = torch.randn(Out, In, generator=g) * 3 + 1
    pre_b = torch.randn(Out, generator=g) * 3 - 1
    return tuple(t.cuda() for t in (x, w, dy, dyq, pre_w, pre_b))


@functools.lru_cache(maxsize=None)
def _bwd_ref(B, In, Out):
    """float64 dW, db of dyq and the magnitudes their bounds need."""
    x, _, _, dyq, _, _ = _bwd_inputs(B, In, Out)
    x64, d64 = x.cpu().double(), dyq.cpu().double()
    return dict(dw=d64.T @ x64, dw_S=d64.abs().T @ x64.abs(),
                db=d64.sum(0), db_S=d64.abs().sum(0))


def _run_bwd(dy, x, w, pre_w, pre_b, accum, with_db, with_dx):
    """One linear_bwd call; accum hands in copies of the initial buffers."""
    dw_out = pre_w.clone() if accum else None
    db_out = pre_b.clone() if (accum and with_db) else None
    dx, dw, db = _C().linear_bwd(dy, x, w, with_dx, with_db, dw_out, db_out)
    torch.cuda.synchronize()
    if accum:
        assert dw.data_ptr() == dw_out.data_ptr()
    return dx, dw, db


@pytest.mark.parametrize("Out", BWD_OUT)
@pytest.mark.parametrize("In", BWD_IN)
@pytest.mark.parametrize("B", BWD_B)
def test_bwd_fused(B, In, Out):
    """Every variant of one shape: dx bitwise the two-kernel path's, dW/db
    bitwise repeatable and within the summation bound of float64."""
    x, w, dy, dyq, pre_w, pre_b = _bwd_inputs(B, In, Out)
    r = _bwd_ref(B, In, Out)
    worst = 0.0
    for accum, with_db, with_dx in VARIANTS:
        tag = f"[{B},{In},{Out}] accum={accum} db={with_db} dx={with_dx}"
        with _switch("linear_bwd_fused", True):
            dx, dw, db = _run_bwd(dy, x, w, pre_w, pre_b, accum, with_db,
                                  with_dx)
            dx2, dw2, db2 = _run_bwd(dy, x, w, pre_w, pre_b, accum, with_db,
                                     with_dx)
            _, dwq, dbq = _run_bwd(dyq, x, w, pre_w, pre_b, accum, with_db,
                                   False)
        with _switch("linear_bwd_fused", False):
            dx_old = _run_bwd(dy, x, w, pre_w, pre_b, accum, with_db,
                              with_dx)[0]
        assert (dx is None) == (not with_dx), tag
        assert (db is None) == (not with_db), tag
        if with_dx:
            assert dx.dtype == torch.bfloat16 and dx.shape == (B, In)
            assert float(dx.float().abs().max()) > 0.0, tag
            assert torch.equal(dx, dx_old), (
                f"{tag}: {int((dx != dx_old).sum())} dx elements differ")
            assert torch.equal(dx, dx2), tag
        assert torch.equal(dw, dw2), tag + ": dW differs between two calls"
        if with_db:
            assert torch.equal(db, db2), tag + ": db differs between calls"
        # float64, per element
        ref_w, bnd_w = r["dw"], B * U * r["dw_S"]
        ref_b, bnd_b = r["db"], B * U * r["db_S"]
        if accum:
            p_w, p_b = pre_w.cpu().double(), pre_b.cpu().double()
            ref_w, bnd_w = ref_w + p_w, bnd_w + _ulp(p_w)
            ref_b, bnd_b = ref_b + p_b, bnd_b + _ulp(p_b)
        err = (dwq.cpu().double() - ref_w).abs()
        worst = max(worst, float((err / bnd_w.clamp_min(1e-300)).max()))
        assert bool((err <= bnd_w).all()), f"{tag}: dW {worst:.3f} x bound"
        if with_db:
            err = (dbq.cpu().double() - ref_b).abs()
            worst = max(worst, float((err / bnd_b.clamp_min(1e-300)).max()))
            assert bool((err <= bnd_b).all()), f"{tag}: db {worst:.3f} x bound"
    print(f"linear_bwd_small [{B},{In},{Out}]: max |err|/bound = {worst:.3f}")


@pytest.mark.parametrize("B,In,Out", [(64, 512, 10), (3, 1032, 16),
                                      (128, 24, 1)])
def test_bwd_deterministic_mode_keeps_old_kernels(B, In, Out):
    """Deterministic mode with the switch on gives, bitwise, what the
    two-kernel path gives with it off (dx, dW, db), into fresh buffers and
    accumulating."""
    x, w, dy, _, pre_w, pre_b = _bwd_inputs(B, In, Out)
    for accum in (0, 1):
        with _switch("linear_bwd_fused", False):
            old = _run_bwd(dy, x, w, pre_w, pre_b, accum, True, True)
        with _switch("linear_bwd_fused", True), _switch("deterministic", True):
            det = _run_bwd(dy, x, w, pre_w, pre_b, accum, True, True)
        for what, a, b in zip(("dx", "dW", "db"), det, old):
            assert torch.equal(a, b), f"[{B},{In},{Out}] accum={accum} {what}"


@pytest.mark.parametrize("B,In,Out", [(64, 512, 10), (3, 1032, 16)])
def test_bwd_graph_replay_equals_eager(B, In, Out):
    """The accumulating call captured once, replayed on three new sets of
    inputs: each replay bitwise the eager call on the same inputs."""
    C = _C()
    x0, w0, dy0, _, pre_w, pre_b = _bwd_inputs(B, In, Out)
    sx, sw, sdy = x0.clone(), w0.clone(), dy0.clone()
    sdw, sdb = pre_w.clone(), pre_b.clone()
    with _switch("linear_bwd_fused", True):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            C.linear_bwd(sdy, sx, sw, True, True, sdw, sdb)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            sdx = C.linear_bwd(sdy, sx, sw, True, True, sdw, sdb)[0]
        g = torch.Generator().manual_seed(7)
        for rep in range(3):
            x = torch.randn(B, In, generator=g).bfloat16().cuda()
            w = (torch.randn(Out, In, generator=g) * 0.1).bfloat16().cuda()
            dy = (torch.randn(B, Out, generator=g) * 0.3).cuda()
            for dst, src in ((sx, x), (sw, w), (sdy, dy), (sdw, pre_w),
                             (sdb, pre_b)):
                dst.copy_(src)
            graph.replay()
            torch.cuda.synchronize()
            dx, dw, db = _run_bwd(dy, x, w, pre_w, pre_b, 1, True, True)
            assert torch.equal(sdx, dx), f"replay {rep}: dx"
            assert torch.equal(sdw, dw), f"replay {rep}: dW"
            assert torch.equal(sdb, db), f"replay {rep}: db"
            assert not torch.equal(sdw, pre_w)


# -------------------------------------------------------- cross-entropy -----
def _ce(lg, tg, eps):
    C = _C()
    if eps == 0.0:
        return C.cross_entropy_fwd_bwd(lg, tg)
    return C.cross_entropy_ls_fwd_bwd(lg, tg, eps)


def _ce_inputs(B, NC):
    g = torch.Generator().manual_seed(B * 31 + NC)
    return ((torch.randn(B, NC, generator=g) * 3).cuda(),
            torch.randint(0, NC, (B,), generator=g).cuda())


def _poison_free_list():
    """Leave 1e30 in the blocks the allocator hands out next for a scalar
    and for small outputs, so a loss that was added to stale memory shows."""
    junk = [torch.full((n,), 1e30, device="cuda") for n in (1, 1, 1, 128)]
    torch.cuda.synchronize()
    del junk


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("NC", [2, 10])
@pytest.mark.parametrize("B", [1, 64, 256])
def test_ce_store_equals_zeroed_add_bitwise(B, NC, eps):
    lg, tg = _ce_inputs(B, NC)
    with _switch("ce_store", False):
        loss_old, d_old = _ce(lg, tg, eps)
        torch.cuda.synchronize()
    with _switch("ce_store", True):
        _poison_free_list()
        loss, d = _ce(lg, tg, eps)
        torch.cuda.synchronize()
    assert loss.dim() == 0 and 0.0 < float(loss) < 100.0
    assert torch.equal(d, d_old)
    assert torch.equal(loss, loss_old), (
        f"[{B},{NC}] eps={eps}: {float(loss)!r} vs {float(loss_old)!r}")


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_ce_above_one_workgroup_keeps_the_add_form(eps):
    """B = 300 launches two workgroups: the switch changes nothing, the loss
    is added into a zeroed scalar.  That form's loss depends, in its last
    bits, on the order in which the workgroups' atomics land, so the value is
    held to what the same form gives over four launches, widened by the
    5 wave partials' worth of reordering (5 * u * loss); dlogits is
    bitwise."""
    B, NC = 300, 10
    lg, tg = _ce_inputs(B, NC)
    with _switch("ce_store", False):
        olds = [_ce(lg, tg, eps) for _ in range(4)]
    with _switch("ce_store", True):
        _poison_free_list()
        loss, d = _ce(lg, tg, eps)
    torch.cuda.synchronize()
    assert torch.equal(d, olds[0][1])
    vals = [float(lo) for lo, _ in olds]
    tol = 5 * U * max(vals)
    assert min(vals) - tol <= float(loss) <= max(vals) + tol
