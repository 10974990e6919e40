"""Per-element float64 tests for the depthwise, pool, classifier and
cross-entropy kernels, in default and deterministic mode.

Every case feeds a kernel the exact bf16 / f32 values it sees, computes the
same operation on the CPU in float64 and compares PER ELEMENT against a bound
tensor derived from the kernel's code.  With ``u = 2^-8`` (bf16 unit
roundoff), ``e = 2^-24`` (f32) and ``A`` the same linear map applied to
absolute values:

* f32 output of a length-K accumulation:          ``D·e·A``
* bf16 output of an exact selection / copy:       bitwise equal
* bf16 output of an f32 computation:              ``u·|ref| + D·e·A``
* bf16 output computed from a bf16 intermediate:  ``2u·A + u·|ref|``

``D`` is the accumulation depth read off the kernel, rounded up to a power
of two.  Two outputs need a term beyond these, both found by measuring and
explained where they are used: the BN-backward ``dconv`` can cancel to zero,
so the depthwise dx/dw bounds carry the f32 error of its terms, and the
cross-entropy argument carries the f32 rounding of ``lse`` itself.

Tiled and vectorised dimensions carry large-magnitude sentinels
(±5…7) in their first and last element so that a dropped tail breaks the
bound at every output it feeds.  The worst measured ``|err| / bound`` per
group is recorded in docs/VALIDATION_LOG.md.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -8    # bf16 unit roundoff
E = 2.0 ** -24   # f32 unit roundoff


def _C():
    from horizonml_amd import ops
    return ops.extension()


@pytest.fixture(params=[False, True], ids=["default", "det"])
def det(request):
    """Run the test body in default and in deterministic mode."""
    if request.param:
        _C().set_deterministic(True)
    try:
        yield request.param
    finally:
        _C().set_deterministic(False)


def _pow2(n):
    return 1 << max(0, math.ceil(math.log2(max(1, n))))


def _gen(*key):
    """A CPU generator seeded by the case, so every case has its own data."""
    seed = 17
    for k in key:
        seed = (seed * 1000003 + int(k) + 1) % (2 ** 31 - 1)
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def _spike(t, *dims):
    """Sentinels: the first and last slice of each listed dim get distinct
    large magnitudes (5…6 and 6…7, all bf16-exact), signs kept."""
    for d in dims:
        for pos, base in ((0, 5.0), (t.shape[d] - 1, 6.0)):
            sl = t.select(d, pos)
            mag = base + (torch.arange(sl.numel()) % 5).reshape(sl.shape) \
                .to(t.dtype) * 0.25
            sl.copy_(torch.where(sl >= 0, mag, -mag))
    return t


def _check(got, ref, bound, what):
    """|got − ref| ≤ bound at every element; prints the worst ratio."""
    got = got.detach().double().cpu()
    ref = ref.double()
    bound = bound.double().expand_as(ref)
    assert got.shape == ref.shape, f"{what}: {got.shape} vs {ref.shape}"
    err = (got - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300),
                        torch.where(err > 0, torch.full_like(err, math.inf),
                                    torch.zeros_like(err)))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"RATIO {what} {worst:.4f}")
    bad = err > bound
    assert not bool(bad.any()), (
        f"{what}: {int(bad.sum())}/{bad.numel()} elements out of bound, "
        f"worst |err|/bound = {worst:.3f}")
    return worst


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def _cl(t):
    """[N,C,H,W] CPU tensor -> bf16 channels_last on the GPU."""
    return t.to(torch.bfloat16).cuda().contiguous(
        memory_format=torch.channels_last)


# ================================================================ linear ===
LIN_FWD_CASES = [
    (1, 8, 1),         # one chunk, one live lane
    (5, 504, 10),      # chunk = 63: lane 63 idle; one live wave in block 2
    (4, 512, 16),
    (3, 520, 17),      # chunk = 65: t = 1 has a single live lane
    (7, 1280, 10),     # per_lane = 3, MobileNet head
    (2, 2048, 1000),   # per_lane = 4 full, ImageNet head
]


def _lin_inputs(B, In, Out, seed=0):
    g = _gen(B, In, Out, seed)
    x = _spike(torch.randn(B, In, generator=g), 0, 1).bfloat16()
    w = _spike(torch.randn(Out, In, generator=g), 0, 1).bfloat16()
    b = _spike(torch.randn(Out, generator=g), 0)
    return x, w, b


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("B,In,Out", LIN_FWD_CASES)
def test_linear_fwd(B, In, Out, with_bias):
    x, w, b = _lin_inputs(B, In, Out)
    y = _C().linear_fwd(x.cuda(), w.cuda(), b.cuda() if with_bias else None)
    assert y.dtype == torch.float32 and tuple(y.shape) == (B, Out)
    ref = x.double() @ w.double().T
    A = x.double().abs() @ w.double().abs().T
    if with_bias:
        ref = ref + b.double()
        A = A + b.double().abs()
    # <= 32 fmas per lane + 6 shuffle adds + bias = 39 -> D = 64
    _check(y, ref, 64 * E * A, f"linear_fwd[{B},{In},{Out}]")


def test_linear_fwd_guards():
    C = _C()

    def xw(B, In, Out, In_w=None):
        return (torch.zeros(B, In).bfloat16().cuda(),
                torch.zeros(Out, In_w or In).bfloat16().cuda())

    with pytest.raises(RuntimeError, match="2048"):
        C.linear_fwd(*xw(2, 2056, 3), None)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        C.linear_fwd(*xw(2, 12, 3), None)
    with pytest.raises(RuntimeError, match="input columns"):
        C.linear_fwd(*xw(2, 16, 3, In_w=24), None)
    with pytest.raises(RuntimeError, match="bias"):
        C.linear_fwd(*xw(2, 16, 3), torch.zeros(4).cuda())
    x, w = xw(2, 16, 3)
    with pytest.raises(RuntimeError):
        C.linear_fwd(x, w.cpu(), None)
    with pytest.raises(RuntimeError):
        C.linear_fwd(x, w.reshape(3, 2, 8), None)


LIN_BWD_CASES = [
    # (B, In, Out, deterministic)
    (1, 8, 1, False),        # small
    (5, 264, 10, False),     # small: two blocks, 8 live threads in the 2nd
    (128, 520, 16, False),   # small, at both limits
    (129, 512, 10, False),   # bsplit: second chunk is a single row
    (300, 264, 16, False),   # bsplit, three chunks
    (5, 24, 17, False),      # generic
    (130, 40, 17, False),    # generic
    (300, 264, 10, True),    # deterministic: must take the generic kernel
    (64, 512, 10, True),     # deterministic, small
]


def _lin_bwd_refs(dy, x, w):
    dy64, x64, w64 = dy.double(), x.double(), w.double()
    return dict(
        dw=dy64.T @ x64, dw_A=dy64.abs().T @ x64.abs(),
        db=dy64.sum(0), db_A=dy64.abs().sum(0),
        dx=dy64 @ w64, dx_A=dy64.abs() @ w64.abs())


@pytest.mark.parametrize("direct", [False, True], ids=["fresh", "direct"])
@pytest.mark.parametrize("B,In,Out,deterministic", LIN_BWD_CASES)
def test_linear_bwd(B, In, Out, deterministic, direct):
    C = _C()
    x, w, _ = _lin_inputs(B, In, Out, seed=1)
    g = _gen(B, In, Out, 2)
    dy = _spike(torch.randn(B, Out, generator=g), 0, 1)
    r = _lin_bwd_refs(dy, x, w)
    pre_w = torch.randn(Out, In, generator=g) * 3 + 1
    pre_b = torch.randn(Out, generator=g) * 3 - 1
    dw_out = pre_w.cuda() if direct else None
    db_out = pre_b.cuda() if direct else None
    if deterministic:
        C.set_deterministic(True)
    try:
        dx, dw, db = C.linear_bwd(dy.cuda(), x.cuda(), w.cuda(), True, True,
                                  dw_out, db_out)
        torch.cuda.synchronize()
    finally:
        C.set_deterministic(False)
    tag = f"linear_bwd[{B},{In},{Out},det={int(deterministic)}," \
          f"direct={int(direct)}]"
    D = _pow2(B + 8)
    dw_ref, db_ref = r["dw"], r["db"]
    dw_b, db_b = D * E * r["dw_A"], D * E * r["db_A"]
    if direct:
        # result = prefill + gradient, written into the given buffers
        assert dw.data_ptr() == dw_out.data_ptr()
        assert db.data_ptr() == db_out.data_ptr()
        dw_ref, db_ref = dw_ref + pre_w.double(), db_ref + pre_b.double()
        dw_b = dw_b + E * pre_w.double().abs()
        db_b = db_b + E * pre_b.double().abs()
    assert dw.dtype == torch.float32 and db.dtype == torch.float32
    _check(dw, dw_ref, dw_b, tag + ".dw")
    _check(db, db_ref, db_b, tag + ".db")
    assert dx.dtype == torch.bfloat16
    _check(dx, r["dx"], U * r["dx"].abs() + Out * E * r["dx_A"], tag + ".dx")


@pytest.mark.parametrize("B,In,Out", [(5, 264, 10), (129, 512, 10),
                                      (5, 24, 17)])
def test_linear_bwd_optional_outputs(B, In, Out):
    """need_dx = False / need_db = False return None for that output and
    leave the others right, on each dW route."""
    C = _C()
    x, w, _ = _lin_inputs(B, In, Out, seed=3)
    dy = _spike(torch.randn(B, Out, generator=_gen(B, In, Out, 4)), 0, 1)
    r = _lin_bwd_refs(dy, x, w)
    D = _pow2(B + 8)
    dx, dw, db = C.linear_bwd(dy.cuda(), x.cuda(), w.cuda(), False, True,
                              None, None)
    assert dx is None
    _check(dw, r["dw"], D * E * r["dw_A"], f"linear_bwd_nodx[{B}].dw")
    _check(db, r["db"], D * E * r["db_A"], f"linear_bwd_nodx[{B}].db")
    dx, dw, db = C.linear_bwd(dy.cuda(), x.cuda(), w.cuda(), True, False,
                              None, None)
    assert db is None
    _check(dw, r["dw"], D * E * r["dw_A"], f"linear_bwd_nodb[{B}].dw")
    _check(dx, r["dx"], U * r["dx"].abs() + Out * E * r["dx_A"],
           f"linear_bwd_nodb[{B}].dx")
    # direct mode without a bias gradient: dW accumulates, db stays absent
    pre = torch.full((Out, In), 2.5)
    dx, dw, db = C.linear_bwd(dy.cuda(), x.cuda(), w.cuda(), False, False,
                              pre.cuda(), None)
    assert dx is None and db is None
    _check(dw, r["dw"] + 2.5, D * E * r["dw_A"] + E * 2.5,
           f"linear_bwd_direct_nodb[{B}].dw")


def test_linear_bwd_guards():
    C = _C()
    B, In, Out = 4, 16, 3
    dy = torch.zeros(B, Out).cuda()
    x = torch.zeros(B, In).bfloat16().cuda()
    w = torch.zeros(Out, In).bfloat16().cuda()
    with pytest.raises(RuntimeError, match="dy must be"):
        C.linear_bwd(torch.zeros(B, Out + 1).cuda(), x, w, True, True, None,
                     None)
    with pytest.raises(RuntimeError, match="dy must be"):
        C.linear_bwd(torch.zeros(B + 1, Out).cuda(), x, w, True, True, None,
                     None)
    with pytest.raises(RuntimeError, match="x must be"):
        C.linear_bwd(dy, x.float(), w, True, True, None, None)
    with pytest.raises(RuntimeError, match="input columns"):
        C.linear_bwd(dy, x, torch.zeros(Out, In + 8).bfloat16().cuda(), True,
                     True, None, None)
    with pytest.raises(RuntimeError, match="dw_out"):
        C.linear_bwd(dy, x, w, True, True, torch.zeros(In, Out).cuda(), None)
    with pytest.raises(RuntimeError, match="dw_out"):  # not contiguous
        C.linear_bwd(dy, x, w, True, True, torch.zeros(In, Out).cuda().T,
                     None)
    with pytest.raises(RuntimeError, match="dw_out"):  # not f32
        C.linear_bwd(dy, x, w, True, True,
                     torch.zeros(Out, In).bfloat16().cuda(), None)
    with pytest.raises(RuntimeError, match="db_out"):
        C.linear_bwd(dy, x, w, True, True, torch.zeros(Out, In).cuda(),
                     torch.zeros(Out + 1).cuda())


# ========================================================= cross-entropy ===
# Constant of the CE bound.  __expf/__logf under -ffast-math have no error
# bound derivable from the source, so c is set from the measurement on an
# MI355X: worst observed |err|/bound against the float64 reference at c = 1,
# times 2 (docs/VALIDATION_LOG.md).  The worst element is a target-class
# gradient near −1 at B = 3: (p − q)·fl(1/B) rounds twice at that size, which
# the absolute c·e term has to carry.
CE_C = 2 * 1.6216

CE_SHAPES = [(1, 2), (5, 10), (300, 10), (257, 32), (3, 1000)]


def _ce_inputs(B, NC, scale):
    g = _gen(B, NC, int(scale))
    logits = torch.randn(B, NC, generator=g) * scale
    target = torch.randint(0, NC, (B,), generator=g)
    # special rows, as many as the batch holds: a 200-wide gap (every other
    # class underflows to p = 0) with the target on an underflowed class, an
    # all-equal row, target 0 and target NC − 1
    rows = list(range(min(B, 4)))
    if len(rows) > 0:
        r = rows[-1]
        logits[r] = torch.randn(NC, generator=g)
        logits[r, NC // 2] += 200.0
        target[r] = (NC // 2 + 1) % NC
    if len(rows) > 1:
        logits[0] = 1.5 * scale
        target[0] = 0
    if len(rows) > 2:
        target[1] = NC - 1
    if len(rows) > 3:
        target[2] = 0
    return logits, target


def _ce_ref(logits, target, eps, eps_div=None, b_div=None):
    """float64 loss, G = B·dlogits and their bounds (at c = 1).  eps_div and
    b_div replace NC in ε/NC and B in 1/B (the perturbed references)."""
    B, NC = logits.shape
    x = logits.double()
    eps_div = NC if eps_div is None else eps_div
    b_div = B if b_div is None else b_div
    lsm = F.log_softmax(x, dim=1)
    p = lsm.exp()
    onehot = F.one_hot(target, NC).double()
    # ε/NC on every class plus (1 − ε) on the target; with eps_div = NC this
    # is F.cross_entropy's label_smoothing
    off = eps / eps_div if eps > 0 else 0.0
    q = (1 - eps) * onehot + off
    li = -(q * lsm).sum(1)
    inv_b = 1.0 / b_div
    loss = li.sum() * inv_b
    G = (p - q) * (B * inv_b)
    # p_j = exp(row_j − lse) with lse = log(Σ) + max held in f32: the
    # argument carries the rounding of the subtraction, |row_j − lse|·e, AND
    # of lse itself, |lse|·e — the kernel's softmax is shift-invariant only
    # to f32 precision of the logits' magnitude.  (Without the |lse| term
    # the scale-30 cases measured 12.8x the bound at p ≈ 1, |lse| ≈ 80.)
    lse = torch.logsumexp(x, 1)
    Gb = (lsm.abs() + lse.abs()[:, None] + 4) * E * p + E
    xt = x.gather(1, target[:, None])[:, 0]
    # loss: the log argument is a sum of NC exps (NC·e), lse = log + max and
    # lse − x_t round at their own magnitude, the smoothing term sums the
    # row (NC·e·mean|row|); rows then accumulate in f32 (pow2(B + 8) deep)
    per_row = E * (NC + 4 + 2 * lse.abs() + 2 * xt.abs() + 4 * li.abs()
                   + eps * (NC + 4) * x.abs().mean(1))
    lb = per_row.mean() + _pow2(B + 8) * E * li.abs().mean()
    return loss, G, lb, Gb


def _ce_call(logits, target, eps):
    C = _C()
    lg, tg = logits.cuda(), target.cuda()
    if eps == 0:
        return C.cross_entropy_fwd_bwd(lg, tg)
    return C.cross_entropy_ls_fwd_bwd(lg, tg, eps)


@pytest.mark.parametrize("scale", [1.0, 30.0], ids=["s1", "s30"])
@pytest.mark.parametrize("eps", [0.0, 0.1], ids=["onehot", "ls"])
@pytest.mark.parametrize("B,NC", CE_SHAPES)
def test_cross_entropy(B, NC, eps, scale, det):
    logits, target = _ce_inputs(B, NC, scale)
    loss, dlogits = _ce_call(logits, target, eps)
    assert loss.dtype == torch.float32 and dlogits.dtype == torch.float32
    loss_ref, G_ref, lb, Gb = _ce_ref(logits, target, eps)
    tag = f"ce[{B},{NC},eps={eps},s={int(scale)},det={int(det)}]"
    got_G = dlogits.double().cpu() * B
    got_loss = loss.double().cpu()
    _check(got_loss, loss_ref, CE_C * lb, tag + ".loss")
    # absolute comparison: p_j may underflow in f32
    _check(got_G, G_ref, CE_C * Gb, tag + ".G")

    # the bound must be tight enough to tell the formula from its near
    # misses: ε/(NC−1) instead of ε/NC, 1/(B−1) instead of 1/B
    def violates(lr, Gr):
        return bool(((got_loss - lr).abs() > CE_C * lb)
                    or ((got_G - Gr).abs() > CE_C * Gb).any())

    if eps > 0:
        lr, Gr, _, _ = _ce_ref(logits, target, eps, eps_div=NC - 1)
        assert violates(lr, Gr), f"{tag}: eps/(NC-1) reference is in bound"
    if B > 1:  # at B = 1 the perturbed reference is infinite
        lr, Gr, _, _ = _ce_ref(logits, target, eps, b_div=B - 1)
        assert violates(lr, Gr), f"{tag}: 1/(B-1) reference is in bound"

    if det:  # ordered reduction: the loss is bitwise reproducible
        loss2, dl2 = _ce_call(logits, target, eps)
        assert torch.equal(loss, loss2) and torch.equal(dlogits, dl2)


@pytest.mark.parametrize("eps", [0.0, 0.1], ids=["onehot", "ls"])
def test_cross_entropy_autograd_scales_grad(eps):
    from horizonml_amd.models._functional_gpu import cross_entropy
    logits, target = _ce_inputs(5, 10, 1.0)
    _, dlogits = _ce_call(logits, target, eps)
    lg = logits.cuda().requires_grad_(True)
    loss = cross_entropy(lg, target.cuda(), label_smoothing=eps)
    (3 * loss).backward()
    assert torch.equal(lg.grad, dlogits * 3)


# ================================================================= pools ===
MAXPOOL_CASES = [
    (2, 8, 1, 1), (1, 16, 2, 3), (2, 24, 5, 7), (1, 64, 8, 6),   # v8
    (2, 3, 5, 7), (1, 20, 6, 6), (3, 12, 4, 9),                  # scalar
]


def _maxpool_input(family, shape):
    g = _gen(*shape, len(family))
    if family == "randn":
        x = torch.randn(shape, generator=g)
    elif family == "ties":
        x = torch.randint(-3, 4, shape, generator=g).float()
    elif family == "negative":       # padding must never win
        x = -torch.rand(shape, generator=g) - 0.5
    elif family == "huge_negative":  # every value finite and below -1e30
        x = -(1.5 + 1.5 * torch.rand(shape, generator=g)) * 1e38
    else:
        raise ValueError(family)
    return x.bfloat16()


def _maxpool_ref(x):
    """3x3 / stride 2 / pad 1 max-pool by a plain scan: the first maximum in
    (r, s) order among the in-bounds taps (torch's own rule)."""
    x = x.float().numpy()
    N, C, H, W = x.shape
    Hp, Wp = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = np.zeros((N, C, Hp, Wp), np.float32)
    idx = np.full((N, C, Hp, Wp), -1, np.int64)
    for ho in range(Hp):
        for wo in range(Wp):
            for r in range(3):
                hi = ho * 2 - 1 + r
                if hi < 0 or hi >= H:
                    continue
                for s in range(3):
                    wi = wo * 2 - 1 + s
                    if wi < 0 or wi >= W:
                        continue
                    v = x[:, :, hi, wi]
                    take = (idx[:, :, ho, wo] < 0) | (v > y[:, :, ho, wo])
                    y[:, :, ho, wo] = np.where(take, v, y[:, :, ho, wo])
                    idx[:, :, ho, wo] = np.where(take, r * 3 + s,
                                                 idx[:, :, ho, wo])
    return y, idx


def _maxpool_bwd_ref(dy, idx, H, W):
    dy = dy.float().numpy()
    N, C, Hp, Wp = dy.shape
    dx = np.zeros((N, C, H, W), np.float32)
    for ho in range(Hp):
        for wo in range(Wp):
            k = idx[:, :, ho, wo]
            hi, wi = ho * 2 - 1 + k // 3, wo * 2 - 1 + k % 3
            n, c = np.meshgrid(np.arange(N), np.arange(C), indexing="ij")
            np.add.at(dx, (n, c, hi, wi), dy[:, :, ho, wo])
    return dx


@pytest.mark.parametrize("family", ["randn", "ties", "negative",
                                    "huge_negative"])
@pytest.mark.parametrize("shape", MAXPOOL_CASES,
                         ids=lambda s: "x".join(map(str, s)))
def test_maxpool_fwd_bwd(shape, family):
    N, Cn, H, W = shape
    x = _maxpool_input(family, shape)
    assert bool(torch.isfinite(x.float()).all())
    y_ref, idx_ref = _maxpool_ref(x)
    assert idx_ref.min() >= 0
    y, idx = _C().maxpool_fwd(_cl(x))
    assert y.dtype == torch.bfloat16 and idx.dtype == torch.uint8
    # exact selection: bitwise equal, argmax equal everywhere
    assert torch.equal(_bits(y), _bits(torch.from_numpy(y_ref).bfloat16()))
    assert tuple(idx.shape) == (N, y_ref.shape[2], y_ref.shape[3], Cn)
    got_idx = idx.cpu().permute(0, 3, 1, 2).long().numpy()
    assert np.array_equal(got_idx, idx_ref)

    # backward with small-integer dy: every sum is exact in bf16
    dy = torch.randint(-3, 4, y_ref.shape, generator=_gen(*shape, 7)) \
        .float().bfloat16()
    dx = _C().maxpool_bwd(_cl(dy), idx, H, W)
    assert tuple(dx.shape) == shape and dx.dtype == torch.bfloat16
    dx_ref = torch.from_numpy(_maxpool_bwd_ref(dy, idx_ref, H, W))
    assert torch.equal(dx.float().cpu(), dx_ref)
    assert torch.equal(dx.float().cpu().sum((2, 3)), dy.float().sum((2, 3)))


AVGPOOL_CASES = [(2, 8, 1, 1), (3, 20, 2, 2), (2, 5, 3, 3), (2, 512, 7, 7),
                 (1, 24, 2, 5)]


@pytest.mark.parametrize("shape", AVGPOOL_CASES,
                         ids=lambda s: "x".join(map(str, s)))
def test_avgpool_fwd_bwd(shape):
    N, Cn, H, W = shape
    g = _gen(*shape)
    x = _spike(torch.randn(shape, generator=g), 0, 1, 2, 3).bfloat16()
    y = _C().avgpool_fwd(_cl(x))
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (N, Cn)
    x64 = x.double()
    ref = x64.mean((2, 3))
    _check(y, ref, U * ref.abs() + H * W * E * x64.abs().mean((2, 3)),
           f"avgpool_fwd{list(shape)}")
    dy = _spike(torch.randn(N, Cn, generator=g), 0, 1).bfloat16()
    dx = _C().avgpool_bwd(dy.cuda(), H, W)
    assert dx.dtype == torch.bfloat16 and tuple(dx.shape) == shape
    dref = (dy.double() / (H * W))[:, :, None, None].expand(shape)
    _check(dx, dref, U * dref.abs(), f"avgpool_bwd{list(shape)}")


# ====================================================== depthwise conv+BN ===
DW_CASES = [
    # (N, C, H, W, R=S, stride, pad)
    (2, 8, 5, 5, 3, 1, 1),
    (1, 32, 8, 8, 3, 2, 1),
    (2, 96, 9, 7, 3, 2, 1),    # 64+32 channel tail block, H != W, odd/s2
    (1, 72, 6, 6, 5, 1, 2),    # R*S = 25 = DW_MAXRS
    (3, 144, 4, 4, 3, 1, 1),
    (1, 64, 1, 1, 3, 1, 1),    # every tap but the centre is padded
    (2, 20, 7, 5, 3, 2, 1),    # C % 8 != 0: flat BN path
]
DW_MOMENTUM, DW_EPS = 0.1, 1e-5


def _dw_inputs(case):
    N, Cn, H, W, R, s, p = case
    g = _gen(*case)
    sdims = (0, 1, 2, 3) if N >= 3 else (1, 2, 3)
    x = _spike(torch.randn(N, Cn, H, W, generator=g), *sdims).bfloat16()
    w = _spike(torch.randn(R, R, Cn, generator=g), 2).bfloat16()
    gamma = 0.5 + torch.rand(Cn, generator=g)
    beta = torch.randn(Cn, generator=g)
    rm0 = 0.1 * torch.randn(Cn, generator=g)
    rv0 = 0.5 + torch.rand(Cn, generator=g)
    Ho, Wo = (H + 2 * p - R) // s + 1, (W + 2 * p - R) // s + 1
    dy = _spike(torch.randn(N, Cn, Ho, Wo, generator=g), *sdims).bfloat16()
    return x, w, gamma, beta, rm0, rv0, dy


def _dw_fwd(case, inp):
    x, w, gamma, beta, rm0, rv0, _ = inp
    rm, rv = rm0.clone().cuda(), rv0.clone().cuda()
    out = _C().dw_conv_bn_fwd(_cl(x), w.cuda(), gamma.cuda(), beta.cuda(),
                              rm, rv, case[5], case[6], DW_MOMENTUM, DW_EPS,
                              True, 0, None)
    torch.cuda.synchronize()
    return out, rm, rv


def _w_oihw(w):
    return w.double().permute(2, 0, 1).unsqueeze(1).contiguous()  # [C,1,R,S]


@pytest.mark.parametrize("case", DW_CASES,
                         ids=lambda c: "x".join(map(str, c)))
def test_dw_conv_bn_fwd(case, det):
    N, Cn, H, W, R, s, p = case
    inp = _dw_inputs(case)
    x, w, gamma, beta, rm0, rv0, _ = inp
    (y, convout, smean, sinvstd), rm, rv = _dw_fwd(case, inp)
    tag = f"dw_fwd{list(case)}det={int(det)}"
    x64, w4 = x.double(), _w_oihw(w)
    ref = F.conv2d(x64, w4, None, s, p, 1, Cn)
    A = F.conv2d(x64.abs(), w4.abs(), None, s, p, 1, Cn)
    assert convout.dtype == torch.bfloat16
    # at most 25 fmas -> D = 32
    _check(convout, ref, U * ref.abs() + 32 * E * A, tag + ".convout")

    # --- batch statistics, against the kernel's own returned convout ------
    cv = convout.double().cpu()
    M = N * cv.shape[2] * cv.shape[3]
    D = _pow2(M + 8)
    S1, A1 = cv.sum((0, 2, 3)), cv.abs().sum((0, 2, 3))
    S2 = (cv * cv).sum((0, 2, 3))
    mean = S1 / M
    var = (S2 / M - mean * mean).clamp_min(0)
    # Default mode sums the unrounded f32 accumulator a = cv·(1+θ), |θ| ≤ u,
    # so Σa is within u·Σ|cv| of Σcv and Σa² within (2u+u²)·Σcv²;
    # deterministic mode sums the rounded tensor itself.  Both sums then
    # carry D·e of f32 accumulation error.
    ur = 0.0 if det else U
    d_mean = (D * E + ur) * A1 / M + 2 * E * mean.abs()
    # var = Σx²/M − mean²: first-order propagation plus the f32 roundings of
    # the two products and the subtraction
    d_var = ((D * E + 2 * ur + ur * ur) * S2 / M
             + 2 * mean.abs() * d_mean + d_mean * d_mean
             + 4 * E * (S2 / M + mean * mean))
    _check(smean, mean, d_mean, tag + ".smean")
    # invstd = (var + eps)^-1/2 is monotone: bound it by its value at both
    # ends of the var interval, plus 4e for rsqrtf itself
    istd = (var + DW_EPS).rsqrt()
    istd_hi = ((var - d_var).clamp_min(0) + DW_EPS).rsqrt()
    istd_lo = (var + d_var + DW_EPS).rsqrt()
    d_istd = torch.maximum(istd_hi - istd, istd - istd_lo) + 4 * E * istd
    _check(sinvstd, istd, d_istd, tag + ".sinvstd")

    # --- running statistics: one update, unbiased variance ---------------
    ub = M / (M - 1) if M > 1 else 1.0
    rm_ref = (1 - DW_MOMENTUM) * rm0.double() + DW_MOMENTUM * mean
    rv_ref = (1 - DW_MOMENTUM) * rv0.double() + DW_MOMENTUM * var * ub
    _check(rm, rm_ref, DW_MOMENTUM * d_mean
           + 4 * E * (rm0.double().abs() + mean.abs()), tag + ".running_mean")
    _check(rv, rv_ref, DW_MOMENTUM * ub * d_var
           + 4 * E * (rv0.double().abs() + var * ub), tag + ".running_var")

    # --- y: the affine map on the returned convout and statistics --------
    # y = a·x + b, a = γ·invstd, b = β − mean·a (v8) or (x − mean)·invstd·γ
    # + β (flat): four to five f32 roundings on terms of size a·|x|, a·|mean|
    # and |β|, so D = 8 on A = |a|·(|x| + |mean|) + |β|; then one bf16
    # rounding
    sm = smean.double().cpu()[None, :, None, None]
    si = sinvstd.double().cpu()[None, :, None, None]
    ga = gamma.double()[None, :, None, None]
    be = beta.double()[None, :, None, None]
    y_ref = (cv - sm) * si * ga + be
    y_A = (ga * si).abs() * (cv.abs() + sm.abs()) + be.abs()
    assert y.dtype == torch.bfloat16
    _check(y, y_ref, U * y_ref.abs() + 8 * E * y_A, tag + ".y")


@pytest.mark.parametrize("case", DW_CASES,
                         ids=lambda c: "x".join(map(str, c)))
def test_dw_conv_bn_bwd(case, det):
    N, Cn, H, W, R, s, p = case
    inp = _dw_inputs(case)
    x, w, gamma, beta, _, _, dy = inp
    (y, convout, smean, sinvstd), _, _ = _dw_fwd(case, inp)
    dx, dw, sum_dzx, sum_dz, dres = _C().dw_conv_bn_bwd(
        _cl(dy), y, _cl(x), w.cuda(), convout, gamma.cuda(), beta.cuda(),
        smean, sinvstd, s, p, 0, True, False)
    torch.cuda.synchronize()
    tag = f"dw_bwd{list(case)}det={int(det)}"
    # reference dconv by the BN-backward formula from dy and the forward's
    # returned convout / statistics (each checked by the forward test), so
    # that the depthwise dgrad and wgrad are isolated from BN rounding
    cv = convout.double().cpu()
    Ho, Wo = cv.shape[2], cv.shape[3]
    M = N * Ho * Wo
    sm = smean.double().cpu()[None, :, None, None]
    si = sinvstd.double().cpu()[None, :, None, None]
    ga = gamma.double()[None, :, None, None]
    dz = dy.double()
    xh = (cv - sm) * si
    r_dz, r_dzx = dz.sum((0, 2, 3)), (dz * xh).sum((0, 2, 3))
    D = _pow2(M + 8)
    b_dz = D * E * dz.abs().sum((0, 2, 3))
    b_dzx = D * E * (dz * xh).abs().sum((0, 2, 3))
    _check(sum_dz, r_dz, b_dz, tag + ".sum_dz")
    _check(sum_dzx, r_dzx, b_dzx, tag + ".sum_dzx")
    m_dz = r_dz[None, :, None, None] / M
    m_dzx = r_dzx[None, :, None, None] / M
    dconv = ga * si * (dz - m_dz - xh * m_dzx)
    # dconv is a difference of three terms scaled by γ·invstd and can cancel
    # completely (at M = 1 it is exactly 0, while each term is ~300·|dy|):
    # the kernel's f32 evaluation (A·dz + E − D·x, at most 8 roundings) and
    # its own channel sums (within b_dz, b_dzx of the reference, above) err
    # relative to the TERMS, not to the result.  F carries that floor
    # through dgrad and wgrad; away from cancellation it is ~2^-13 of the
    # 2u·A term.
    F32 = (ga * si).abs() * (
        8 * E * (dz.abs() + m_dz.abs()
                 + si * (cv.abs() + sm.abs()) * m_dzx.abs())
        + (b_dz[None, :, None, None] + xh.abs() * b_dzx[None, :, None, None])
        / M)

    w4 = _w_oihw(w)
    op = (H - ((Ho - 1) * s - 2 * p + R), W - ((Wo - 1) * s - 2 * p + R))
    dx_ref = F.conv_transpose2d(dconv, w4, None, s, p, op, Cn)
    dx_A = F.conv_transpose2d(dconv.abs(), w4.abs(), None, s, p, op, Cn)
    dx_F = F.conv_transpose2d(F32, w4.abs(), None, s, p, op, Cn)
    assert dx.dtype == torch.bfloat16 and tuple(dx.shape) == (N, Cn, H, W)
    _check(dx, dx_ref, 2 * U * dx_A + U * dx_ref.abs() + dx_F, tag + ".dx")

    # dw[r,s,c] = Σ_{n,ho,wo} x[n,c,ho·s−p+r,wo·s−p+s]·dconv[n,c,ho,wo]
    xp = F.pad(x.double(), (p, p, p, p))
    dw_ref = torch.zeros(R, R, Cn).double()
    dw_A = torch.zeros(R, R, Cn).double()
    dw_F = torch.zeros(R, R, Cn).double()
    for r in range(R):
        for q in range(R):
            xs = xp[:, :, r:r + (Ho - 1) * s + 1:s, q:q + (Wo - 1) * s + 1:s]
            dw_ref[r, q] = (xs * dconv).sum((0, 2, 3))
            dw_A[r, q] = (xs * dconv).abs().sum((0, 2, 3))
            dw_F[r, q] = (xs.abs() * F32).sum((0, 2, 3))
    assert dw.dtype == torch.float32 and tuple(dw.shape) == (R, R, Cn)
    _check(dw, dw_ref, 2 * U * dw_A + _pow2(M // 4 + 8) * E * dw_A + dw_F,
           tag + ".dw")


def test_dw_conv_bn_guards():
    """A 7x7 depthwise filter (49 taps > 25) is refused by both entry
    points before any launch, as are a zero stride and an empty output."""
    C = _C()
    N, Cn, H, W = 1, 8, 8, 8
    x = _cl(torch.zeros(N, Cn, H, W))
    f = torch.zeros(Cn).cuda()
    rm, rv = torch.zeros(Cn).cuda(), torch.ones(Cn).cuda()
    w7 = torch.zeros(7, 7, Cn).bfloat16().cuda()
    w3 = torch.zeros(3, 3, Cn).bfloat16().cuda()

    def fwd(w, stride, pad, xx=x):
        return C.dw_conv_bn_fwd(xx, w, f, f, rm, rv, stride, pad, 0.1, 1e-5,
                                True, 0, None)

    def bwd(w, stride, pad, ho, wo):
        d = _cl(torch.zeros(N, Cn, ho, wo))
        return C.dw_conv_bn_bwd(d, d, x, w, d, f, f, f, f, stride, pad, 0,
                                True, False)

    with pytest.raises(RuntimeError, match="R\\*S <= 25"):
        fwd(w7, 1, 3)
    with pytest.raises(RuntimeError, match="R\\*S <= 25"):
        bwd(w7, 1, 3, 8, 8)
    with pytest.raises(RuntimeError, match="stride"):
        fwd(w3, 0, 1)
    with pytest.raises(RuntimeError, match="stride"):
        bwd(w3, 0, 1, 8, 8)
    with pytest.raises(RuntimeError, match="at least 1x1"):
        fwd(torch.zeros(5, 5, Cn).bfloat16().cuda(), 1, 0,
            xx=_cl(torch.zeros(N, Cn, 4, 4)))
    with pytest.raises(RuntimeError, match="\\[R,S,C\\]"):
        bwd(torch.zeros(3, 3, Cn + 8).bfloat16().cuda(), 1, 1, 8, 8)
    with pytest.raises(RuntimeError, match="\\[R,S,C\\]"):
        bwd(torch.zeros(3, 3, 1, Cn).bfloat16().cuda(), 1, 1, 8, 8)
    with pytest.raises(RuntimeError, match="dy shape"):
        bwd(w3, 1, 1, 4, 4)
    assert bool((rm == 0).all()) and bool((rv == 1).all())
