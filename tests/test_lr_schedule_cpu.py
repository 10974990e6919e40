"""Host side of the device-resident LR schedules: ``LRSchedule.lr_at`` against
closed forms and torch's schedulers (both float64), the float32 table, the
label-smoothing forward on CPU, and the checkpoint round-trip of the
scheduled SGD's step counter on a stand-in manager."""
import math
import types

import pytest
import torch
import torch.nn.functional as F

from horizonml_amd.engine.schedule import LRSchedule, schedule_from_epochs

# Both sides compute in float64; 1e-9 is orders of magnitude looser than
# double rounding and only avoids == on floats.
RTOL = 1e-9


def _close(a, b):
    return abs(a - b) <= RTOL * max(abs(a), abs(b), 1e-300)


def _torch_lrs(make_sched, base_lr, n):
    """lr used by update t = 0..n-1 when the scheduler steps once per update
    (float64 throughout: param_groups hold Python floats)."""
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=base_lr)
    sched = make_sched(opt)
    out = []
    for _ in range(n):
        out.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    return out


def test_warmup_matches_lambdalr():
    base, T, W = 0.1, 20, 7
    s = LRSchedule("constant", base, T, warmup_steps=W)
    ref = _torch_lrs(lambda o: torch.optim.lr_scheduler.LambdaLR(
        o, lambda t: min(1.0, (t + 1) / W)), base, T)
    for t in range(T):
        assert _close(s.lr_at(t), ref[t]), (t, s.lr_at(t), ref[t])
        if t < W:
            assert _close(s.lr_at(t), base * (t + 1) / W)
    assert s.lr_at(W - 1) == base


@pytest.mark.parametrize("min_lr", [0.0, 1e-4])
def test_cosine_matches_closed_form(min_lr):
    base, T = 0.1, 50
    s = LRSchedule("cosine", base, T, min_lr=min_lr)
    # CosineAnnealingLR's closed form (its chained recursion drifts by
    # rounding, _get_closed_form_lr is the definition)
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=base)
    cos = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=T,
                                                     eta_min=min_lr)
    for t in range(T):
        cos.last_epoch = t
        ref = cos._get_closed_form_lr()[0]
        mine = min_lr + (base - min_lr) * 0.5 * (1 + math.cos(
            math.pi * t / T))
        assert _close(s.lr_at(t), ref), (t, s.lr_at(t), ref)
        assert _close(s.lr_at(t), mine)


def test_cosine_after_warmup():
    base, T, W = 0.2, 30, 5
    s = LRSchedule("cosine", base, T, warmup_steps=W, min_lr=0.01)
    for t in range(W, T):
        p = (t - W) / (T - W)
        ref = 0.01 + (base - 0.01) * 0.5 * (1 + math.cos(math.pi * p))
        assert _close(s.lr_at(t), ref)
    assert s.lr_at(W) == base  # p = 0 right after the warm-up


def test_linear_closed_form():
    base, T, W = 0.3, 12, 2
    s = LRSchedule("linear", base, T, warmup_steps=W, min_lr=0.03)
    for t in range(W, T):
        p = (t - W) / (T - W)
        assert _close(s.lr_at(t), base + (0.03 - base) * p)


def test_multistep_matches_torch():
    base, T, ms, gamma = 0.1, 25, [5, 11, 11, 20], 0.3
    s = LRSchedule("multistep", base, T, milestones=ms, gamma=gamma)
    ref = _torch_lrs(lambda o: torch.optim.lr_scheduler.MultiStepLR(
        o, milestones=ms, gamma=gamma), base, T)
    for t in range(T):
        assert _close(s.lr_at(t), ref[t]), (t, s.lr_at(t), ref[t])


def test_edge_cases():
    # no warm-up: update 0 already runs at base_lr
    assert LRSchedule("cosine", 0.1, 10).lr_at(0) == 0.1
    assert LRSchedule("constant", 0.1, 10).lr_at(9) == 0.1
    # warm-up spans the whole run: pure ramp, ends at base_lr
    s = LRSchedule("cosine", 0.1, 8, warmup_steps=8)
    for t in range(8):
        assert _close(s.lr_at(t), 0.1 * (t + 1) / 8)
    # past the end: holds the last value
    for kind in ("constant", "cosine", "linear", "multistep"):
        s = LRSchedule(kind, 0.1, 10, warmup_steps=3, min_lr=0.01,
                       milestones=[4, 8])
        assert s.lr_at(10) == s.lr_at(9)
        assert s.lr_at(10 ** 6) == s.lr_at(9)
    # min_lr == base_lr: flat
    for kind in ("cosine", "linear"):
        s = LRSchedule(kind, 0.1, 10, min_lr=0.1)
        assert all(_close(s.lr_at(t), 0.1) for t in range(10))
    # a milestone at t = 0 applies to the first update
    s = LRSchedule("multistep", 0.1, 10, milestones=[0, 5], gamma=0.5)
    assert _close(s.lr_at(0), 0.05) and _close(s.lr_at(5), 0.025)


def test_constructor_rejects():
    with pytest.raises(ValueError):
        LRSchedule("cosine", 0.1, 0)
    with pytest.raises(ValueError):
        LRSchedule("cosine", 0.1, 2 ** 24)
    with pytest.raises(ValueError):
        LRSchedule("cosine", 0.1, 2 ** 24 + 5)
    LRSchedule("cosine", 0.1, 2 ** 24 - 1)  # the largest exact counter
    with pytest.raises(ValueError):
        LRSchedule("exponential", 0.1, 10)
    with pytest.raises(ValueError):
        LRSchedule("cosine", 0.1, 10, warmup_steps=-1)


@pytest.mark.parametrize("kind", ["constant", "cosine", "linear",
                                  "multistep"])
def test_table_is_float32_of_lr_at(kind):
    s = LRSchedule(kind, 0.1, 37, warmup_steps=4, min_lr=1e-3,
                   milestones=[10, 20], gamma=0.1)
    tab = s.table()
    assert tab.dtype == torch.float32 and tab.shape == (37,)
    for i in range(37):
        want = torch.tensor(s.lr_at(i), dtype=torch.float64) \
            .to(torch.float32)
        assert tab[i].item() == want.item(), i


def test_schedule_from_epochs():
    s = schedule_from_epochs("multistep", 0.1, epochs=10, steps_per_epoch=7,
                             warmup_epochs=1, milestones=[3, 6], gamma=0.1)
    assert s.total_steps == 70 and s.warmup_steps == 7
    assert s.milestones == (21, 42)
    from horizonml_amd.engine.common import build_schedule
    assert build_schedule("constant", 0.1, 10, 7) is None  # today's path
    assert build_schedule("constant", 0.1, 10, 7,
                          warmup_epochs=1).warmup_steps == 7
    assert build_schedule("cosine", 0.1, 10, 7).total_steps == 70


def test_label_smoothing_cpu_forwards_to_torch():
    from horizonml_amd.models._functional_gpu import cross_entropy
    torch.manual_seed(0)
    logits = torch.randn(9, 10) * 3
    y = torch.randint(0, 10, (9,))
    a = logits.clone().requires_grad_(True)
    b = logits.clone().requires_grad_(True)
    la = cross_entropy(a, y, label_smoothing=0.1)
    lb = F.cross_entropy(b, y, label_smoothing=0.1)
    la.backward(), lb.backward()
    assert torch.equal(la, lb) and torch.equal(a.grad, b.grad)
    assert torch.equal(cross_entropy(logits, y), F.cross_entropy(logits, y))
    assert not torch.equal(la.detach(), F.cross_entropy(logits, y))


def test_eager_optimizer_knobs():
    from horizonml_amd.engine.common import build_optimizer
    p = [torch.nn.Parameter(torch.zeros(3))]
    o = build_optimizer(p, "sgd", lr=0.1, weight_decay=5e-4, nesterov=True)
    assert o.defaults["nesterov"] and o.defaults["weight_decay"] == 5e-4
    o = build_optimizer(p, "adam", weight_decay=1e-2, decoupled_wd=True)
    assert isinstance(o, torch.optim.AdamW)
    o = build_optimizer(p, "adam")
    assert type(o) is torch.optim.Adam and o.defaults["weight_decay"] == 0.0


def test_scheduled_sgd_step_t_checkpoint_roundtrip(tmp_path):
    from horizonml_amd.engine.flat import HorizonAdam, HorizonSGD
    from horizonml_amd.utils.checkpoint import (load_checkpoint,
                                                save_checkpoint)
    mgr = types.SimpleNamespace(master=torch.arange(8, dtype=torch.float32))
    sched = LRSchedule("cosine", 0.1, 40, warmup_steps=4)
    model = torch.nn.Linear(2, 2)
    path = str(tmp_path / "sgd.pt")

    sgd = HorizonSGD(mgr, lr=0.1, momentum=0.9, schedule=sched,
                     nesterov=True)
    assert torch.equal(sgd.lr_table, sched.table())
    assert sgd.lr_table.device == mgr.master.device
    with torch.no_grad():
        sgd.mom.copy_(torch.randn(8))
    sgd.set_step(23)
    save_checkpoint(path, model, sgd, epoch=1)
    sgd2 = HorizonSGD(mgr, lr=0.1, momentum=0.9, schedule=sched)
    load_checkpoint(path, model, sgd2)
    assert float(sgd2.step_t) == 23.0
    assert torch.equal(sgd2.mom, sgd.mom)

    # a state dict from before SGD kept a counter: loads, counter untouched
    old = HorizonSGD(mgr, lr=0.1, momentum=0.9)
    assert old.step_t is None and "step_t" not in old.state_dict()
    sgd3 = HorizonSGD(mgr, lr=0.1, momentum=0.9, schedule=sched)
    sgd3.set_step(11)
    sgd3.load_state_dict(old.state_dict())
    assert float(sgd3.step_t) == 11.0
    # and a scheduled checkpoint loads into an unscheduled optimizer
    old.load_state_dict(sgd.state_dict())
    assert torch.equal(old.mom, sgd.mom)
    old.set_step(5)  # no counter to position: a no-op
    assert old.current_lr() == 0.1

    adam = HorizonAdam(mgr, lr=2e-3, schedule=sched, decoupled_wd=True)
    adam.set_step(7)
    save_checkpoint(path, model, adam, epoch=1)
    adam2 = HorizonAdam(mgr, lr=2e-3, schedule=sched)
    load_checkpoint(path, model, adam2)
    assert float(adam2.step_t) == 7.0
    assert HorizonAdam(mgr, lr=2e-3).current_lr() == 2e-3
    with pytest.raises(ValueError):
        HorizonSGD(mgr, momentum=0.0, nesterov=True)
