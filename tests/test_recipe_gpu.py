"""GPU side of the device-resident LR schedule and the recipe knobs of the
fused step (``k_adam_step_ex`` / ``k_sgd_step_ex``, Nesterov, AdamW, label
smoothing in the fused cross-entropy).

The reference for the scheduled kernels is the existing ``sgd_step`` /
``adam_step`` op driven eagerly with ``float(table[t])`` per step: it sees the
same float32 lr and evaluates the same expression, so equality is bitwise.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from horizonml_amd.engine.schedule import LRSchedule

pytestmark = pytest.mark.gpu

MU, WD = 0.9, 5e-4
B1, B2, EPS = 0.9, 0.999, 1e-8


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


def _cosine_table(T=5, warmup=2, base=0.1):
    return LRSchedule("cosine", base, T, warmup_steps=warmup).table()


def _grads(n, steps, seed, dyadic=False):
    """A fresh randn gradient per step; ``dyadic`` rounds it to multiples of
    1/8 (see test_scheduled_adam_equals_existing_op_bitwise)."""
    g = torch.Generator().manual_seed(seed)
    out = [torch.randn(n, generator=g) for _ in range(steps)]
    if dyadic:
        out = [(x * 8).round() / 8 for x in out]
    return [x.to(_dev()) for x in out]


class _SGDState:
    def __init__(self, master0):
        self.master = master0.clone()
        self.grad = torch.zeros_like(master0)
        self.mom = torch.zeros_like(master0)
        self.shadow = torch.zeros_like(master0, dtype=torch.bfloat16)

    def tensors(self):
        return self.master, self.grad, self.mom, self.shadow


class _AdamState:
    def __init__(self, master0):
        self.master = master0.clone()
        self.grad = torch.zeros_like(master0)
        self.m = torch.zeros_like(master0)
        self.v = torch.zeros_like(master0)
        self.shadow = torch.zeros_like(master0, dtype=torch.bfloat16)
        self.step_t = torch.zeros(1, device=master0.device)
        self.extra = torch.ones(37, device=master0.device)

    def tensors(self):
        return self.master, self.grad, self.m, self.v, self.shadow


def _assert_same(a, b, names):
    for x, y, nm in zip(a, b, names):
        assert torch.equal(x, y), f"{nm} not bitwise equal"


# ------------------------------------------------ scheduled == existing op --
@pytest.mark.parametrize("n", [1, 4099])
def test_scheduled_sgd_equals_existing_op_bitwise(ext, n):
    table = _cosine_table()
    T = table.numel()
    dtab = table.to(_dev())
    torch.manual_seed(n)
    master0 = torch.randn(n, device=_dev())
    ref, new = _SGDState(master0), _SGDState(master0)
    step_t = torch.zeros(1, device=_dev())
    lr_out = torch.full((1,), -1.0, device=_dev())
    for k, g in enumerate(_grads(n, 8, 10 + n)):   # 3 past the table's end
        ref.grad.copy_(g), new.grad.copy_(g)
        ext.sgd_step(ref.master, ref.grad, ref.mom, ref.shadow,
                     float(table[min(k, T - 1)]), MU, WD, True, None, 1.0,
                     None, None, None)
        # lr=123: must be ignored in favour of the table
        ext.sgd_step_sched(new.master, new.grad, new.mom, new.shadow, step_t,
                           dtab, lr_out, 123.0, MU, WD, False, True)
        _assert_same(new.tensors(), ref.tensors(),
                     ("master", "grad", "mom", "shadow"))
        assert lr_out.item() == table[min(k, T - 1)].item(), k
        assert step_t.item() == k + 1
    assert float(new.grad.abs().sum()) == 0.0


@pytest.mark.parametrize("variant", ["probe", "probe_randn", "grad_bf16"])
def test_scheduled_adam_equals_existing_op_bitwise(ext, variant):
    """``probe``: the fused divergence probe ends in one float atomicAdd per
    block (17 blocks at n = 4099), whose order varies run to run — measured
    on an MI355X, the existing ``adam_step`` against ITSELF on identical
    randn inputs gives a different probe output in 67 of 300 steps (new
    against existing: 57 of 300; master / m / v / prev: 0 of 300 both ways).
    So for the bitwise check of the probe output the gradients are randn
    rounded to multiples of 1/8: every (g - prev)^2 and every partial sum is
    then exact in f32 (an integer count of 1/64ths, about 2^19 in total, far
    below 2^24) and the order cannot matter.  ``probe_randn`` keeps unrounded randn gradients with the probe
    on and checks everything but that one scalar."""
    n = 4099
    table = _cosine_table()
    T = table.numel()
    dtab = table.to(_dev())
    torch.manual_seed(7)
    master0 = torch.randn(n, device=_dev())
    ref, new = _AdamState(master0), _AdamState(master0)
    lr_out = torch.full((1,), -1.0, device=_dev())
    probes = [None, None]
    probe_on = variant.startswith("probe")
    dyadic = variant == "probe"
    if probe_on:
        prev0 = _grads(n, 1, 20, dyadic)[0]
        probes = [(prev0.clone(), torch.zeros(1, device=_dev()),
                   torch.zeros(1, device=_dev())) for _ in range(2)]
    for k, g in enumerate(_grads(n, 8, 21, dyadic)):
        ref.grad.copy_(g), new.grad.copy_(g)
        ref.extra.fill_(1.0), new.extra.fill_(1.0)
        gb, gs = None, 1.0
        if variant == "grad_bf16":
            gb, gs = (g * 2).to(torch.bfloat16), 0.5
        pr = probes[0] if probes[0] is not None else (None, None, None)
        pn = probes[1] if probes[1] is not None else (None, None, None)
        ext.adam_step(ref.master, ref.grad, ref.m, ref.v, ref.shadow,
                      ref.step_t, float(table[min(k, T - 1)]), B1, B2, EPS,
                      WD, True, ref.extra, gb, gs, *pr)
        ext.adam_step_sched(new.master, new.grad, new.m, new.v, new.shadow,
                            new.step_t, dtab, lr_out, 123.0, B1, B2, EPS, WD,
                            False, True, new.extra, gb, gs, *pn)
        _assert_same(new.tensors(), ref.tensors(),
                     ("master", "grad", "m", "v", "shadow"))
        assert torch.equal(new.step_t, ref.step_t)
        assert float(new.extra.abs().sum()) == 0.0
        assert lr_out.item() == table[min(k, T - 1)].item(), k
        if probe_on:
            assert torch.equal(probes[1][0], probes[0][0])       # prev
            assert torch.equal(probes[1][0], g)
            assert float(probes[1][1]) == 0.0                    # sumsq reset
            assert float(probes[1][2]) > 0.0
        if variant == "probe":
            assert torch.equal(probes[1][2], probes[0][2]), k    # output


def test_constant_schedule_equals_float_lr_bitwise(ext):
    n = 4099
    dtab = LRSchedule("constant", 0.05, 3).table().to(_dev())
    torch.manual_seed(3)
    master0 = torch.randn(n, device=_dev())
    rs, ns = _SGDState(master0), _SGDState(master0)
    ra, na = _AdamState(master0), _AdamState(master0)
    step_t = torch.zeros(1, device=_dev())
    lr_out = torch.zeros(1, device=_dev())
    for g in _grads(n, 4, 33):
        for s in (rs, ns, ra, na):
            s.grad.copy_(g)
        ext.sgd_step(rs.master, rs.grad, rs.mom, rs.shadow, 0.05, MU, WD,
                     True, None, 1.0, None, None, None)
        ext.sgd_step_sched(ns.master, ns.grad, ns.mom, ns.shadow, step_t,
                           dtab, lr_out, 123.0, MU, WD, False, True)
        ext.adam_step(ra.master, ra.grad, ra.m, ra.v, ra.shadow, ra.step_t,
                      0.05, B1, B2, EPS, WD, True, None, None, 1.0, None,
                      None, None)
        ext.adam_step_sched(na.master, na.grad, na.m, na.v, na.shadow,
                            na.step_t, dtab, None, 123.0, B1, B2, EPS, WD,
                            False, True)
    _assert_same(ns.tensors(), rs.tensors(),
                 ("master", "grad", "mom", "shadow"))
    _assert_same(na.tensors(), ra.tensors(),
                 ("master", "grad", "m", "v", "shadow"))
    assert lr_out.item() == dtab[0].item()


def test_unscheduled_ex_kernel_uses_float_lr(ext):
    """No table: the extended kernels take ``lr`` by value (the path of
    Nesterov / AdamW without a schedule) and bump no SGD counter."""
    n = 4099
    torch.manual_seed(4)
    master0 = torch.randn(n, device=_dev())
    rs, ns = _SGDState(master0), _SGDState(master0)
    lr_out = torch.zeros(1, device=_dev())
    for g in _grads(n, 2, 34):
        rs.grad.copy_(g), ns.grad.copy_(g)
        ext.sgd_step(rs.master, rs.grad, rs.mom, rs.shadow, 0.05, MU, WD,
                     True, None, 1.0, None, None, None)
        ext.sgd_step_sched(ns.master, ns.grad, ns.mom, ns.shadow, None, None,
                           lr_out, 0.05, MU, WD, False, True)
    _assert_same(ns.tensors(), rs.tensors(),
                 ("master", "grad", "mom", "shadow"))
    assert lr_out.item() == torch.tensor(0.05).item()


def test_sched_argument_checks(ext):
    n = 8
    s = _SGDState(torch.zeros(n, device=_dev()))
    step_t = torch.zeros(1, device=_dev())
    tab = torch.ones(4, device=_dev())

    def call(step_t_=step_t, tab_=tab, lr_out=None, nesterov=False,
             mom=s.mom):
        ext.sgd_step_sched(s.master, s.grad, mom, s.shadow, step_t_, tab_,
                           lr_out, 0.1, MU, 0.0, nesterov, True)

    with pytest.raises(RuntimeError):
        call(tab_=tab.cpu())
    with pytest.raises(RuntimeError):
        call(tab_=tab.double())
    with pytest.raises(RuntimeError):
        call(tab_=torch.ones(0, device=_dev()))
    with pytest.raises(RuntimeError):
        call(step_t_=None)                      # a table needs the counter
    with pytest.raises(RuntimeError):
        call(lr_out=torch.zeros(2, device=_dev()))
    with pytest.raises(RuntimeError):
        call(nesterov=True, mom=None)
    torch.cuda.synchronize()
    assert step_t.item() == 0.0                 # nothing was launched
    call()
    assert step_t.item() == 1.0


# --------------------------------------------------------- graph replay ----
@pytest.mark.parametrize("which", ["sgd", "adam"])
def test_graph_replay_walks_the_table(ext, which):
    """One captured step (counter bump + kernel), replayed past the end of a
    T=4 table: the lr changes per replay with no host work.  On the parent
    the lr is a by-value kernel argument baked into the graph."""
    n, T, R = 4099, 4, 6
    table = _cosine_table(T=T, warmup=1)
    dtab = table.to(_dev())
    torch.manual_seed(9)
    master0 = torch.randn(n, device=_dev())
    grads = _grads(n, R, 44)
    State = _SGDState if which == "sgd" else _AdamState
    ref, new = State(master0), State(master0)
    step_t = new.step_t if which == "adam" else torch.zeros(1, device=_dev())
    lr_out = torch.zeros(1, device=_dev())

    def new_step():
        if which == "sgd":
            ext.sgd_step_sched(new.master, new.grad, new.mom, new.shadow,
                               step_t, dtab, lr_out, 123.0, MU, WD, False,
                               True)
        else:
            ext.adam_step_sched(new.master, new.grad, new.m, new.v,
                                new.shadow, step_t, dtab, lr_out, 123.0, B1,
                                B2, EPS, WD, False, True)

    def ref_step(lr):
        if which == "sgd":
            ext.sgd_step(ref.master, ref.grad, ref.mom, ref.shadow, lr, MU,
                         WD, True, None, 1.0, None, None, None)
        else:
            ext.adam_step(ref.master, ref.grad, ref.m, ref.v, ref.shadow,
                          ref.step_t, lr, B1, B2, EPS, WD, True, None, None,
                          1.0, None, None, None)

    # warm up on a side stream the way train_dp_flat does, then reset
    new.grad.copy_(grads[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        new_step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    fresh = State(master0)
    for t, f in zip(new.tensors(), fresh.tensors()):
        t.copy_(f)
    step_t.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        new_step()
    assert step_t.item() == 0.0 and torch.equal(new.master, master0)

    lrs = []
    for k in range(R):
        new.grad.copy_(grads[k])     # static buffer, new contents
        g.replay()
        lrs.append(lr_out.clone())
        ref.grad.copy_(grads[k])
        ref_step(float(table[min(k, T - 1)]))
    torch.cuda.synchronize()
    names = (("master", "grad", "mom", "shadow") if which == "sgd"
             else ("master", "grad", "m", "v", "shadow"))
    _assert_same(new.tensors(), ref.tensors(), names)
    got =[x.item() for x in lrs]
    assert got == [table[min(k, T - 1)].item() for k in range(R)], got
    assert len(set(got[:T])) > 1     # the schedule really moved
    assert step_t.item() == R


# ------------------------------------------------- Nesterov / AdamW --------
def test_nesterov_matches_torch(ext):
    torch.manual_seed(0)
    n = 4097
    master = torch.randn(n)
    grad = torch.randn(n)
    p = master.clone().requires_grad_(True)
    p.grad = grad.clone()
    opt = torch.optim.SGD([p], lr=0.1, momentum=0.9, nesterov=True,
                          weight_decay=5e-4)
    mg, gg = master.cuda(), grad.cuda()
    mom = torch.zeros(n, device="cuda")
    for _ in range(3):
        opt.step()
        ext.sgd_step_sched(mg, gg, mom, None, None, None, None, 0.1, 0.9,
                           5e-4, True, False)
    r = rel(mg, p.detach())
    print(f"nesterov rel={r:.3e}")
    assert r < 1e-5


def test_adamw_matches_torch(ext):
    torch.manual_seed(0)
    n = 4097
    master = torch.randn(n)
    grad = torch.randn(n)
    p = master.clone().requires_grad_(True)
    p.grad = grad.clone()
    opt = torch.optim.AdamW([p], lr=1e-3, weight_decay=1e-2)
    mg, gg = master.cuda(), grad.cuda()
    m = torch.zeros(n, device="cuda")
    v = torch.zeros(n, device="cuda")
    step_t = torch.zeros(1, device="cuda")
    for _ in range(3):
        opt.step()
        ext.adam_step_sched(mg, gg, m, v, None, step_t, None, None, 1e-3,
                            0.9, 0.999, 1e-8, 1e-2, True, False)
    r = rel(mg, p.detach())
    print(f"adamw rel={r:.3e}")
    assert r < 1e-5


# ----------------------------------------------------- label smoothing -----
@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("B", [5, 300])
def test_label_smoothing(ext, B, det):
    """eps = 0 is today's kernel, bitwise.  eps = 0.1 against fp32 torch: the
    kernels use __expf/__logf, so the bound is measured, not derived — 4x the
    error of the eps = 0 kernel against torch on the same logits (the
    smoothed formula adds one subtraction and one multiply per element to
    the same intrinsics).  The default kernel's loss is a float atomicAdd per
    row, so its last bit depends on the launch: both errors are the worst of
    LAUNCHES launches.  Figures: docs/VALIDATION_LOG.md."""
    from horizonml_amd.models._functional_gpu import cross_entropy
    NC, LAUNCHES = 10, 4
    g = torch.Generator().manual_seed(100 + B)
    logits = torch.randn(B, NC, generator=g) * 3
    y = torch.randint(0, NC, (B,), generator=g)
    lg, yg = logits.to(_dev()), y.to(_dev())

    def torch_ref(eps):
        x = logits.clone().requires_grad_(True)
        loss = F.cross_entropy(x, y, label_smoothing=eps)
        loss.backward()
        return loss.item(), x.grad

    rl0, rd0 = torch_ref(0.0)
    rl1, rd1 = torch_ref(0.1)
    was = ext.deterministic_enabled()
    ext.set_deterministic(det)
    try:
        run0 = [ext.cross_entropy_fwd_bwd(lg, yg) for _ in range(LAUNCHES)]
        run1 = [ext.cross_entropy_ls_fwd_bwd(lg, yg, 0.1)
                for _ in range(LAUNCHES)]
        # eps = 0 through every new entry point: the one-hot kernel
        loss0b, d0b = ext.cross_entropy_ls_fwd_bwd(lg, yg, 0.0)
        x0 = lg.clone().requires_grad_(True)
        l0c = cross_entropy(x0, yg, label_smoothing=0.0)
        l0c.backward()
        x1 = lg.clone().requires_grad_(True)
        l1 = cross_entropy(x1, yg, label_smoothing=0.1)
        l1.backward()
        torch.cuda.synchronize()
    finally:
        ext.set_deterministic(was)
    loss0, d0 = run0[0]
    assert torch.equal(d0b, d0) and torch.equal(x0.grad, d0)
    if det:
        assert torch.equal(loss0b, loss0) and torch.equal(l0c.detach(), loss0)
    assert torch.equal(x1.grad, run1[0][1])
    run1.append((l1.detach(), x1.grad))   # the Python entry point counts too

    e0_d = max((d.cpu() - rd0).abs().max().item() for _, d in run0)
    e0_l = max(abs(lo.item() - rl0) for lo, _ in run0)
    e1_d = max((d.cpu() - rd1).abs().max().item() for _, d in run1)
    e1_l = max(abs(lo.item() - rl1) for lo, _ in run1)
    print(f"label_smoothing B={B} det={det}: eps=0 dlogits {e0_d:.3e} "
          f"loss {e0_l:.3e} | eps=0.1 dlogits {e1_d:.3e} loss {e1_l:.3e} "
          f"| bound dlogits {4 * e0_d:.3e} loss {4 * e0_l:.3e}")
    assert e1_d <= 4 * e0_d
    assert e1_l <= 4 * e0_l


# -------------------------------------------------- through the manager ----
def test_schedule_drives_the_flat_manager(ext):
    """multistep with gamma = 0 from update 2 on: updates 2 and 3 must leave
    the master untouched — the table, not the constructor's lr, drives the
    update on the real flat path."""
    from horizonml_amd.engine.flat import FlatParamManager, HorizonSGD
    from horizonml_amd.models import resnet18
    from horizonml_amd.models._functional_gpu import cross_entropy
    torch.manual_seed(0)
    dev = _dev()
    defer_was = ext.wgrad_defer_enabled()
    try:
        model = resnet18(num_classes=10).to(dev)
        mgr = FlatParamManager(model, dev)
        sched = LRSchedule("multistep", 0.05, 4, milestones=[2], gamma=0.0)
        opt = HorizonSGD(mgr, lr=0.05, schedule=sched)
        x = torch.randn(8, 3, 32, 32, device=dev).to(
            memory_format=torch.channels_last).to(torch.bfloat16)
        y = torch.randint(0, 10, (8,), device=dev)
        start = mgr.master.clone()
        after2 = None
        for k in range(4):
            cross_entropy(model(x), y).backward()
            opt.step()
            if k == 0:
                assert opt.current_lr() == sched.table()[0].item()
            if k == 1:
                after2 = mgr.master.clone()
        assert not torch.equal(after2, start)      # updates 0, 1 trained
        assert torch.equal(mgr.master, after2)     # updates 2, 3 did not
        assert torch.equal(mgr.shadow, after2.to(torch.bfloat16))
        assert opt.current_lr() == 0.0
        assert float(opt.step_t) == 4.0
        assert float(mgr.grad.abs().sum()) == 0.0
        assert ext.wgrad_pending() == 0
    finally:
        ext.set_wgrad_defer(defer_was)


# ---------------------------------------------------- engine end to end ----
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


_RECIPE = dict(lr=0.1, lr_schedule="cosine", warmup_epochs=1,
               weight_decay=5e-4, label_smoothing=0.1, augment=True)


@pytest.mark.timeout(300)
def test_dp_flat_recipe_sgd_end_to_end(tmp_path):
    _run(tmp_path, "sgd", optimizer_name="sgd", nesterov=True, **_RECIPE)


@pytest.mark.timeout(300)
def test_dp_flat_recipe_adamw_end_to_end(tmp_path):
    _run(tmp_path, "adam", optimizer_name="adam", decoupled_wd=True,
         **_RECIPE)
