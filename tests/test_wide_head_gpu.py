"""Wide classifier head (head_kernels.hip): the MFMA linear kernels at
Out > 16 and the wave-per-row cross-entropy at NC > 32, per element against
float64 computed from the same bf16 / f32 inputs.  Helpers, the CE reference
and its bounds are those of test_tail_kernels_gpu.py.
"""
import pytest
import torch

from test_tail_kernels_gpu import (CE_C, E, U, _C, _ce_call, _ce_inputs,
                                   _ce_ref, _check, _gen, _pow2, _spike)

pytestmark = pytest.mark.gpu


def _inputs(B, In, Out, seed):
    g = _gen(B, In, Out, seed)
    x = _spike(torch.randn(B, In, generator=g), 0, 1).bfloat16()
    w = _spike(torch.randn(Out, In, generator=g), 0, 1).bfloat16()
    b = _spike(torch.randn(Out, generator=g), 0)
    # f32 dy, not bf16-representable: a bf16-rounded dy misses the bounds
    dy = _spike(torch.randn(B, Out, generator=g), 0, 1)
    return x, w, b, dy


def _fwd_bound(x, w, b, In):
    # One output's rounding chain: a wave takes every fourth PAIR of 32-k MFMA
    # steps, so 2·ceil(ceil(In/64)/4) steps (16 at In = 2048); 32 products
    # inside a step; 3 combines of the four waves' partials; 1 bias add.
    pairs = -(-In // 64)
    D = _pow2(2 * -(-pairs // 4) + 32 + 3 + 1)
    A = x.double().abs() @ w.double().abs().T
    return D * E * (A + (b.double().abs() if b is not None else 0))


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("B,In,Out", [(1, 8, 17), (17, 40, 33),
                                      (65, 520, 100), (32, 2048, 1000)])
def test_head_fwd(B, In, Out, with_bias):
    x, w, b, _ = _inputs(B, In, Out, 0)
    b = b if with_bias else None
    y = _C().linear_fwd(x.cuda(), w.cuda(), b.cuda() if with_bias else None)
    assert y.dtype == torch.float32 and tuple(y.shape) == (B, Out)
    ref = x.double() @ w.double().T + (b.double() if with_bias else 0)
    _check(y, ref, _fwd_bound(x, w, b, In), f"head_fwd[{B},{In},{Out}]")


def _bwd_check(dy, x, w, got, tag, pre_w=None, pre_b=None):
    """dW/db: pow2(B+8)·e·A (+ e·|prefill|); dx: u·|dx| + Out·e·A — the forms
    of test_tail_kernels_gpu.test_linear_bwd."""
    dx, dw, db = got
    B, Out = dy.shape
    D = _pow2(B + 8)
    dy64, x64, w64 = dy.double(), x.double(), w.double()
    zw = pre_w.double() if pre_w is not None else 0 * (dy64.T @ x64)
    zb = pre_b.double() if pre_b is not None else 0 * dy64.sum(0)
    _check(dw, dy64.T @ x64 + zw,
           D * E * (dy64.abs().T @ x64.abs()) + E * zw.abs(), tag + ".dw")
    if db is not None:
        _check(db, dy64.sum(0) + zb, D * E * dy64.abs().sum(0) + E * zb.abs(),
               tag + ".db")
    if dx is not None:
        assert dx.dtype == torch.bfloat16
        ref = dy64 @ w64
        _check(dx, ref, U * ref.abs() + Out * E * (dy64.abs() @ w64.abs()),
               tag + ".dx")


@pytest.mark.parametrize("det", [False, True], ids=["default", "det"])
@pytest.mark.parametrize("accum", [False, True], ids=["fresh", "accum"])
@pytest.mark.parametrize("B,In,Out", [(1, 8, 17), (5, 24, 33), (33, 72, 65),
                                      (130, 264, 100)])
def test_head_bwd(B, In, Out, accum, det):
    C = _C()
    x, w, _, dy = _inputs(B, In, Out, 1)
    g = _gen(B, In, Out, 2)
    pre_w = torch.randn(Out, In, generator=g) * 3 + 1 if accum else None
    pre_b = torch.randn(Out, generator=g) * 3 - 1 if accum else None
    C.set_deterministic(det)
    try:
        got = C.linear_bwd(dy.cuda(), x.cuda(), w.cuda(), True, True,
                           pre_w.cuda() if accum else None,
                           pre_b.cuda() if accum else None)
        torch.cuda.synchronize()
    finally:
        C.set_deterministic(False)
    _bwd_check(dy, x, w, got, f"head_bwd[{B},{In},{Out},{accum},{det}]",
               pre_w, pre_b)


@pytest.mark.parametrize("need_dx,need_db", [(False, True), (True, False)])
def test_head_bwd_optional_outputs(need_dx, need_db):
    B, In, Out = 33, 72, 65
    x, w, _, dy = _inputs(B, In, Out, 3)
    got = _C().linear_bwd(dy.cuda(), x.cuda(), w.cuda(), need_dx, need_db,
                          None, None)
    assert (got[0] is None) == (not need_dx)
    assert (got[2] is None) == (not need_db)
    _bwd_check(dy, x, w, got, f"head_bwd_opt[dx={need_dx},db={need_db}]")


def test_head_dispatch_and_repeatability():
    C = _C()

    def run(Out):
        x, w, b, dy = (t.cuda() for t in _inputs(5, 24, Out, 4))
        before = C.linear_wide_launches()
        C.linear_fwd(x, w, b)
        out = C.linear_bwd(dy, x, w, True, True, None, None)
        after = C.linear_wide_launches()
        return [a - b for a, b in zip(after, before)], out

    assert C.linear_wide_enabled()
    try:
        rose, out1 = run(17)
        assert rose == [1, 1]
        _, out2 = run(17)
        assert all(torch.equal(a, b) for a, b in zip(out1, out2))
        assert run(16)[0] == [0, 0]
        C.set_linear_wide(False)
        assert not C.linear_wide_enabled() and run(17)[0] == [0, 0]
    finally:
        C.set_linear_wide(True)


@pytest.mark.parametrize("eps", [0.0, 0.1], ids=["onehot", "ls"])
@pytest.mark.parametrize("B,NC", [(1, 33), (5, 100), (70, 1000)])
def test_ce_wide(B, NC, eps):
    assert _C().ce_wide_enabled()
    logits, target = _ce_inputs(B, NC, 1.0)  # carries the special rows
    loss, dlogits = _ce_call(logits, target, eps)
    loss_ref, G_ref, lb, Gb = _ce_ref(logits, target, eps)
    tag = f"ce_wide[{B},{NC},eps={eps}]"
    _check(loss.double().cpu(), loss_ref, CE_C * lb, tag + ".loss")
    _check(dlogits.double().cpu() * B, G_ref, CE_C * Gb, tag + ".G")


def test_head_module_autograd():
    """Linear(64, 100) + cross_entropy through autograd on 8 rows, each stage
    against float64 from that stage's own inputs."""
    from horizonml_amd.models._functional_gpu import cross_entropy
    from horizonml_amd.models.layers import Linear
    torch.manual_seed(5)
    B, In, Out = 8, 64, 100
    lin = Linear(In, Out).cuda()
    x = torch.randn(B, In, generator=_gen(B, In, Out, 5)).bfloat16()
    target = torch.randint(0, Out, (B,), generator=_gen(B, Out, 6))
    xg = x.cuda().requires_grad_(True)
    logits = lin(xg)
    loss = cross_entropy(logits, target.cuda())
    loss.backward()
    w = lin.weight.detach().bfloat16().cpu()
    b = lin.bias.detach().cpu()
    _check(logits, x.double() @ w.double().T + b.double(),
           _fwd_bound(x, w, b, In), "module.logits")
    lg = logits.detach().cpu()
    loss_ref, G_ref, lb, Gb = _ce_ref(lg, target, 0.0)
    _check(loss.detach().double().cpu(), loss_ref, CE_C * lb, "module.loss")
    # the dlogits autograd saved: the same kernel on the same logits
    dl = _C().cross_entropy_fwd_bwd(logits.detach(), target.cuda())[1].cpu()
    _check(dl.double() * B, G_ref, CE_C * Gb, "module.dlogits")
    _bwd_check(dl, x, w, (xg.grad, lin.weight.grad, lin.bias.grad),
               "module.grad")
