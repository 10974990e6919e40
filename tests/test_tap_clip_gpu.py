"""Tap window: forward, dgrad and wgrad skip the filter taps that only ever
meet padding (a 3x3 / pad 1 filter over a 1x1 map has one live tap).

The window is a host-side clip of the conv's geometry (``conv_tap_window``);
the kernels address the full filter from the window's origin.  Checked here:

* the window against a brute-force enumeration of the (output pixel, tap)
  pairs;
* every direction per element against float64 references computed from the
  bf16-rounded operands, with the clip on and off;
* that a clipped wgrad neither reads nor writes the dead taps of ``dW``;
* that a conv with no dead tap computes bitwise what it computes with the
  clip off;
* one ``ConvBNAct`` and one ``BasicBlock`` against the CPU modules.

Bounds.  An output element is an f32 sum of n exact products of bf16 values
(dead products are exact zeros and add nothing), S the sum of their absolute
values.  Any summation order errs by at most n * 2^-24 * S; a bf16 result
adds one rounding, 2^-9 relative, bounded here by 2^-8 * |ref|.  n is counted
per element (the conv of all-ones operands).  Where a sum goes on top of an
earlier f32 value ``prev`` (``dW`` accumulation), ``prev`` is one more term of
the same sum: n additions over the n + 1 terms, n * 2^-24 * (S + |prev|).
"""
import functools
import itertools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _C():
    from horizonml_amd import ops
    return ops.extension()


# (Nb, C, H, W, K, R, stride, pad)
W1 = (4, 16, 1, 1, 16, 3, 1, 1)        # 1x1 window
W2 = (4, 16, 2, 2, 24, 3, 2, 1)        # 2x2 window at origin 1
ROWS = (3, 8, 1, 4, 16, 3, 1, 1)       # rows clipped, columns full: r0 != s0
COLS = (3, 8, 4, 1, 16, 3, 1, 1)       # columns clipped, rows full: r0 != s0
W5 = (2, 16, 1, 1, 8, 5, 1, 2)         # 5x5 -> 1x1 window
SCAL = (2, 3, 2, 2, 16, 7, 2, 3)       # scalar C=3 gather, 2x2 window at 3
ODD = (2, 12, 1, 1, 20, 3, 1, 1)       # C % 8 and K % 8 != 0
SPLIT = (4, 256, 2, 2, 64, 3, 2, 1)    # clipped Kd = 1024: fwd/dgrad split
MSPLIT = (600, 8, 1, 1, 8, 3, 1, 1)    # M = 600: wgrad msplit > 1, clipped
MSPLIT3 = (600, 3, 2, 2, 16, 7, 2, 3)  # ... with C = 3: per-element slab scatter
FULL_PAD = (2, 8, 1, 1, 8, 3, 1, 2)    # Ho = 3, every tap live: no clip
FULL = (2, 16, 4, 4, 16, 3, 1, 1)      # nothing dead

CLIPPED = [W1, W2, ROWS, COLS, W5, SCAL, ODD, SPLIT, MSPLIT, MSPLIT3]
UNCLIPPED = [FULL_PAD, FULL]
SHAPES = CLIPPED + UNCLIPPED


def _out_hw(shape):
    Nb, C, H, W, K, R, stride, pad = shape
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1


class _clip:
    """Sets the switch for a block and puts it back."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.was = _C().tap_clip_enabled()
        _C().set_tap_clip(self.on)

    def __exit__(self, *exc):
        _C().set_tap_clip(self.was)


def _window(shape):
    Nb, C, H, W, K, R, stride, pad = shape
    return tuple(_C().conv_tap_window(H, W, R, R, stride, pad))


def _dead_mask(shape):
    """bool [K, R, S, C]: True on the taps outside the window."""
    Nb, C, H, W, K, R, stride, pad = shape
    r0, s0, Rw, Sw = _window(shape)
    dead = torch.ones(K, R, R, C, dtype=torch.bool)
    dead[:, r0:r0 + Rw, s0:s0 + Sw, :] = False
    return dead


def _msplit(shape, defer):
    """The M split of the shape's clipped wgrad, by the dispatchers' own rules
    (wgrad_msplit for the immediate launch, flush_one_group's 512-row chunks
    for a deferred task with M < 32768)."""
    Nb, C, H, W, K, R, stride, pad = shape
    Ho, Wo = _out_hw(shape)
    M = Nb * Ho * Wo
    _, _, Rw, Sw = _window(shape)
    cdiv = lambda a, b: -(-a // b)  # noqa: E731
    if defer:
        ms = max(1, cdiv(M, 512))
    else:
        tiles = cdiv(Rw * Sw * C, 64) * cdiv(K, 64)
        ms = max(1, min(cdiv(M, 32), 512 // tiles))
    return cdiv(M, cdiv(cdiv(M, ms), 32) * 32)


# ----------------------------------------------------------------- geometry --
def _brute_window(H, W, R, S, stride, pad):
    Ho = (H + 2 * pad - R) // stride + 1
    Wo = (W + 2 * pad - S) // stride + 1
    rows = [r for r in range(R)
            if any(0 <= ho * stride - pad + r < H for ho in range(Ho))]
    cols = [s for s in range(S)
            if any(0 <= wo * stride - pad + s < W for wo in range(Wo))]
    if not rows or not cols:
        # a stride that steps over the whole input (1x1 / stride 2 / pad 3
        # on one pixel): no tap ever meets it; such a conv is left unclipped
        return (0, 0, R, S)
    return (rows[0], cols[0], rows[-1] - rows[0] + 1,
            cols[-1] - cols[0] + 1)


def test_window_matches_enumeration():
    C_ = _C()
    seen = clipped = 0
    for H, W, R, stride, pad in itertools.product(
            range(1, 6), range(1, 6), (1, 3, 5, 7), (1, 2), range(4)):
        if H + 2 * pad < R or W + 2 * pad < R:
            continue  # empty output
        got = tuple(C_.conv_tap_window(H, W, R, R, stride, pad))
        want = _brute_window(H, W, R, R, stride, pad)
        assert got == want, f"{(H, W, R, stride, pad)}: {got} != {want}"
        seen += 1
        clipped += got[2:] != (R, R)
    assert seen > 300 and 0 < clipped < seen


def test_shape_table_windows():
    """The shapes below exercise the windows their names say."""
    assert _window(W1) == (1, 1, 1, 1)
    assert _window(W2) == (1, 1, 2, 2)
    assert _window(ROWS) == (1, 0, 1, 3)
    assert _window(COLS) == (0, 1, 3, 1)
    assert _window(W5) == (2, 2, 1, 1)
    assert _window(SCAL) == (3, 3, 2, 2)
    assert _window(SPLIT) == (1, 1, 2, 2)
    assert _window(MSPLIT3) == (3, 3, 2, 2)
    # the slab paths (vector and per-element scatter) are reached in both modes
    for shape in (MSPLIT, MSPLIT3):
        assert _msplit(shape, False) > 1 and _msplit(shape, True) > 1
    assert _msplit(SCAL, False) == 1 and _msplit(W1, True) == 1
    for shape in UNCLIPPED:
        assert _window(shape) == (0, 0, shape[5], shape[5])


# ----------------------------------------------------- operands, references --
@functools.lru_cache(maxsize=None)
def _operands(shape):
    """Seeded O(1) bf16 operands on the GPU: x, w (KRSC), dz, dx_prev."""
    Nb, C, H, W, K, R, stride, pad = shape
    Ho, Wo = _out_hw(shape)
    g = torch.Generator().manual_seed(
        sum(v * (i + 3) for i, v in enumerate(shape)))
    cl = torch.channels_last
    x = torch.randn(Nb, C, H, W, generator=g)
    w = torch.randn(K, R, R, C, generator=g)
    dz = torch.randn(Nb, K, Ho, Wo, generator=g)
    prev = torch.randn(Nb, C, H, W, generator=g)
    bf = torch.bfloat16
    return (x.cuda().to(memory_format=cl).to(bf), w.cuda().to(bf),
            dz.cuda().to(memory_format=cl).to(bf),
            prev.cuda().to(memory_format=cl).to(bf))


def _triple(fn, a, b):
    """(ref, S, n) of a bilinear conv form in float64."""
    return (fn(a, b), fn(a.abs(), b.abs()),
            fn(torch.ones_like(a), torch.ones_like(b)))


@functools.lru_cache(maxsize=None)
def _refs(shape):
    """float64 (ref, S, n) per direction, NCHW / KRSC, on the CPU."""
    Nb, C, H, W, K, R, stride, pad = shape
    Ho, Wo = _out_hw(shape)
    x, w, dz, prev = (t.cpu().double().contiguous() for t in _operands(shape))
    w_kcrs = w.permute(0, 3, 1, 2).contiguous()
    opad = (H - ((Ho - 1) * stride - 2 * pad + R),
            W - ((Wo - 1) * stride - 2 * pad + R))
    fwd = _triple(lambda a, b: F.conv2d(a, b, stride=stride, padding=pad),
                  x, w_kcrs)
    dgr = _triple(lambda a, b: F.conv_transpose2d(
        a, b, stride=stride, padding=pad, output_padding=opad), dz, w_kcrs)
    wgr = _triple(lambda a, b: torch.nn.grad.conv2d_weight(
        a, (K, C, R, R), b, stride=stride, padding=pad).permute(0, 2, 3, 1),
        x, dz)
    return {"fwd": fwd, "dgrad": dgr, "wgrad": wgr, "prev": prev}


def _check(got, ref, bound, what):
    err = (got.cpu().double() - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: max err/bound = {worst:.3e}")
    assert bool((err <= bound).all()), f"{what}: err/bound = {worst:.3e}"


# ------------------------------------------------------------------ runners --
def _convout(shape):
    C_ = _C()
    Nb, C, H, W, K, R, stride, pad = shape
    x, w, _, _ = _operands(shape)
    f32 = dict(device="cuda", dtype=torch.float32)
    out = C_.conv_bn_act_fwd(x, w, torch.ones(K, **f32), torch.zeros(K, **f32),
                             torch.zeros(K, **f32), torch.ones(K, **f32),
                             stride, pad, 0.1, 1e-5, True, 1, None, None)
    torch.cuda.synchronize()
    return out[1]


def _dx(shape, accum, rsck=False):
    C_ = _C()
    Nb, C, H, W, K, R, stride, pad = shape
    _, w, dz, prev = _operands(shape)
    w_rsck = w.permute(1, 2, 3, 0).contiguous() if rsck else None
    dx = C_.conv_dgrad_only(dz, w, H, W, stride, pad, w_rsck,
                            prev.clone() if accum else None)
    torch.cuda.synchronize()
    return dx


def _dw(shape, defer, dw):
    C_ = _C()
    Nb, C, H, W, K, R, stride, pad = shape
    x, _, dz, _ = _operands(shape)
    got = C_.wgrad_only(x, dz, K, R, R, stride, pad, defer, dw)
    if defer:
        C_.flush_wgrad()
    torch.cuda.synchronize()
    assert got.data_ptr() == dw.data_ptr()
    return dw


# --------------------------------------------------------------- per element --
@pytest.mark.parametrize("clip", [True, False], ids=["clip", "noclip"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_forward_per_element(shape, clip):
    ref, S, n = _refs(shape)["fwd"]
    with _clip(clip):
        got = _convout(shape)
    _check(got, ref, 2.0 ** -8 * ref.abs() + n * 2.0 ** -24 * S,
           f"{shape} clip={clip} convout")


@pytest.mark.parametrize("clip", [True, False], ids=["clip", "noclip"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_dgrad_per_element(shape, clip):
    r = _refs(shape)
    ref, S, n = r["dgrad"]
    with _clip(clip):
        got = _dx(shape, False)
        acc = _dx(shape, True)
    _check(got, ref, 2.0 ** -8 * ref.abs() + n * 2.0 ** -24 * S,
           f"{shape} clip={clip} dx")
    tot = r["prev"] + ref
    _check(acc, tot, 2.0 ** -8 * tot.abs() + n * 2.0 ** -24 * S,
           f"{shape} clip={clip} dx_accum")


@pytest.mark.parametrize("shape", CLIPPED, ids=str)
def test_dgrad_rsck_image_follows_the_window(shape):
    """The RSCK weight image runs the same window, K order and split as the
    KRSC-direct path, so the two stay bitwise equal on clipped convs too."""
    with _clip(True):
        for accum in (False, True):
            direct = _dx(shape, accum)
            legacy = _dx(shape, accum, rsck=True)
            assert torch.equal(direct, legacy), f"{shape} accum={accum}"


@pytest.mark.parametrize("defer", [False, True], ids=["immediate", "deferred"])
@pytest.mark.parametrize("clip", [True, False], ids=["clip", "noclip"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_wgrad_per_element(shape, clip, defer):
    Nb, C, H, W, K, R, stride, pad = shape
    ref, S, n = _refs(shape)["wgrad"]
    with _clip(clip):
        got = _dw(shape, defer, torch.zeros(K, R, R, C, device="cuda"))
    _check(got, ref, n * 2.0 ** -24 * S,
           f"{shape} clip={clip} defer={defer} dW")
    if shape in CLIPPED:
        assert not bool(got.cpu()[_dead_mask(shape)].any())


# --------------------------------------------------------- dead taps untouched --
@pytest.mark.parametrize("defer", [False, True], ids=["immediate", "deferred"])
@pytest.mark.parametrize("shape", CLIPPED, ids=str)
def test_wgrad_leaves_dead_taps(shape, defer):
    """dW pre-filled with a non-zero pattern: the dead taps keep its bits, the
    live taps gain the gradient, and a second call gains it again.  MSPLIT
    and MSPLIT3 take the slab path (msplit > 1, asserted in
    test_shape_table_windows) in both modes, the others write dW from the
    tile epilogue."""
    Nb, C, H, W, K, R, stride, pad = shape
    ref, S, n = _refs(shape)["wgrad"]
    dead = _dead_mask(shape)
    assert bool(dead.any()) and not bool(dead.all())
    pattern = (torch.arange(K * R * R * C, dtype=torch.float32)
               .remainder(13.0).sub(6.5).div(4.0).reshape(K, R, R, C))
    assert not bool((pattern == 0).any())
    pd = pattern.double()
    with _clip(True):
        dw = pattern.cuda()
        for calls in (1, 2):
            _dw(shape, defer, dw)
            got = dw.cpu()
            assert torch.equal(got[dead], pattern[dead]), (
                f"{shape} defer={defer} call {calls}: dead taps written")
            live = ~dead
            bound = calls * n * 2.0 ** -24 * (calls * S + pd.abs())
            _check(got[live], (pd + calls * ref)[live], bound[live],
                   f"{shape} defer={defer} call {calls} live dW")


# ------------------------------------------------------- no clip, no change --
@pytest.mark.parametrize("shape", UNCLIPPED, ids=str)
def test_unclipped_conv_is_bitwise_unchanged(shape):
    Nb, C, H, W, K, R, stride, pad = shape

    def run():
        zeros = lambda: torch.zeros(K, R, R, C, device="cuda")  # noqa: E731
        return [_convout(shape), _dx(shape, False), _dx(shape, True),
                _dw(shape, False, zeros()), _dw(shape, True, zeros())]

    with _clip(True):
        on = run()
    with _clip(False):
        off = run()
    names = ("convout", "dx", "dx_accum", "dW immediate", "dW deferred")
    for name, a, b in zip(names, on, off):
        assert float(b.float().abs().max()) > 0.0
        assert torch.equal(a, b), f"{shape} {name}: clip on != clip off"


# ---------------------------------------------------------------- whole block --
@pytest.fixture(params=[False, True], ids=["default", "det"])
def det(request):
    if request.param:
        _C().set_deterministic(True)
    try:
        yield request.param
    finally:
        _C().set_deterministic(False)


def rel(a, b):
    a = a.float().cpu()
    b = b.float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def to_gpu_cl(x):
    return x.cuda().to(memory_format=torch.channels_last).to(torch.bfloat16)


def _module_pair(kind, cin, cout, stride):
    from horizonml_amd.models.layers import ConvBNAct
    from horizonml_amd.models.resnet import BasicBlock
    torch.manual_seed(0)
    make = ((lambda: ConvBNAct(cin, cout, 3, stride=stride))
            if kind == "conv" else (lambda: BasicBlock(cin, cout, stride)))
    cpu, gpu = make(), make()
    gpu.load_state_dict(cpu.state_dict())
    return cpu, gpu.cuda()


@pytest.mark.parametrize("cfg", [
    # (kind, cin, cout, stride, H = W, bs)
    ("conv", 16, 24, 1, 1, 32),     # 1x1 window
    ("conv", 16, 24, 2, 2, 32),     # 2x2 window at origin 1
    ("block", 32, 32, 1, 1, 32),    # layer4.1 form: both convs 1x1 windows
    ("block", 16, 32, 2, 2, 32),    # layer4.0 form: 2x2 window, 1x1, 1x1/2
], ids=lambda c: "-".join(map(str, c)))
def test_module_fwd_bwd_against_cpu(cfg, det):
    kind, cin, cout, stride, hw, bs = cfg
    cpu, gpu = _module_pair(kind, cin, cout, stride)
    x = torch.randn(bs, cin, hw, hw)
    xc = x.clone().requires_grad_(True)
    xg = to_gpu_cl(x).requires_grad_(True)
    with _clip(True):
        yc = cpu(xc)
        yg = gpu(xg)
        assert yg.shape == yc.shape
        assert rel(yg, yc) < 6e-2, f"y rel={rel(yg, yc)}"
        yc.square().mean().backward()
        yg.float().square().mean().backward()
        torch.cuda.synchronize()
    convs = ([(cpu, gpu)] if kind == "conv" else
             [(getattr(cpu, n), getattr(gpu, n))
              for n in ("conv1", "conv2", "downsample")
              if getattr(cpu, n) is not None])
    for c, g in convs:
        r = rel(g.running_mean, c.running_mean)
        assert r < 3e-2, f"running_mean rel={r}"
        assert rel(g.weight.grad, c.weight.grad) < 6e-2
        assert rel(g.bn_bias.grad, c.bn_bias.grad) < 6e-2
    assert xg.grad.shape == xc.grad.shape
    assert rel(xg.grad, xc.grad) < 6e-2, f"dx rel={rel(xg.grad, xc.grad)}"
