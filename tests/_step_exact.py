"""Exact cases and references for the four kernels that end a training step:
cross-entropy (loss.hip), one-launch SGD (optim.hip), the training max pool
(pool_train.hip) and the bilinear resize forward (resize.hip).  Pure CPU torch
and numpy; tests/test_step_exact_cpu.py proves the references against PyTorch
in float64, tests/test_gpu_step_exact.py holds the kernels to them bit for bit.

Why each family is exact in fp32, whatever the summation order or fma
contraction:

* loss, selection rows: one class holds h in {0..3}, every other -256.  In fp32
  exp(<= -256) = 0, exp(0) = 1, so s = 1, log(s) = 0: the gradient is
  onehot(hot) - onehot(t), a row loss is 0 or 256 + h, and the sum of row
  losses is an integer below 2**24.
* loss, uniform rows: C a power of two <= 4096, every class equal: s = C and
  1 / s are exact, the gradient is 1 / C - onehot(t) (12 bits).  log(C) is not
  exact: the row losses of this family are compared to a tolerance.
* SGD: dyadic hyper-parameters on small integers; every intermediate of the
  header's formula round-trips through float32 (asserted by sgd_reference).
* max pool: the output is a selected input; dx sums at most 225 integers <= 4.
* resize: output = input * 2**j, so the scale, the source coordinates and both
  lambdas are multiples of 2**-6; with |x| <= 100 every product and sum fits
  in 19 bits.

A case that would make a reference inexact fails here, at import or when the
case is built, not silently on the GPU.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np
import torch

import _exact as E

BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
I64 = torch.int64
CL = torch.channels_last
FP32_EXACT = E.FP32_EXACT


def f32_exact(t: torch.Tensor) -> bool:
    """Every element of a float64 tensor survives a trip through float32."""
    return bool(torch.equal(t.to(F32).to(F64), t))


def bf16_exact(t: torch.Tensor) -> bool:
    return bool(torch.equal(t.to(BF).to(F64), t))


# ---- cross-entropy ---------------------------------------------------------------------
XENT_THREADS = 256
OTHER = -256.0  # the logit of every class but the hot one
PAD_COLS = 24   # a padded 2-D view [rows, C] is cut from [rows, C + 24]

# (rows, C) -> the launch path loss.hip's launch() takes
XENT_SHAPES = {
    (1, 2): "narrow", (255, 21): "narrow", (256, 64): "narrow", (257, 21): "narrow", (513, 64): "narrow",
    (1, 65): "small", (64, 65): "small", (3, 4097): "small",
    (65, 65): "wide", (100, 1000): "wide",
}
# 4-D logits [B, C, H, W]: memory format -> shapes
XENT_MAPS = {
    "cl": ((2, 21, 5, 7), (2, 65, 3, 3)),
    "nchw": ((2, 21, 5, 7), (3, 64, 9, 11)),  # 297 rows: more than one narrow block
}
XENT_PADDED = ((257, 21), (64, 65), (65, 65))  # one per launch path
XENT_UNIFORM = ((257, 2), (70, 64), (65, 128), (3, 128), (3, 4096))


def xent_path(rows: int, c: int) -> str:
    """launch()'s two comparisons."""
    if c > 64 and rows <= 64:
        return "small"
    return "wide" if c > 64 else "narrow"


def xent_workspace(rows: int, c: int) -> int:
    """vgpu_cross_entropy_rows_workspace: row losses, and for narrow rows the
    (sum, count) pair of every 256-row block behind them at an even index."""
    if c > 64:
        return rows
    return ((rows + 1) & ~1) + 2 * ((rows + XENT_THREADS - 1) // XENT_THREADS)


def xent_valid(t: torch.Tensor, c: int, ignore: int) -> torch.Tensor:
    return (t >= 0) & (t < c) & (t != ignore)


def xent_narrow_out(loss_rows: torch.Tensor, ok: torch.Tensor, count_spare: bool = False) -> np.ndarray:
    """xent_narrow_kernel's block partials and mean_part_kernel's result, as a
    CPU model: the spare lanes of the ragged last block take row rows - 1 and
    must add nothing.  count_spare: the mistake of counting them (the count
    without its `in &&`)."""
    rows = loss_rows.numel()
    total = cnt = np.float32(0)
    for b0 in range(0, rows, XENT_THREADS):
        lanes = torch.arange(b0, b0 + XENT_THREADS)
        inside = lanes < rows
        row = lanes.clamp_max(rows - 1)
        total += np.float32(float((loss_rows[row] * inside).sum()))
        cnt += np.float32(int((ok[row] & (inside | count_spare)).sum()))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.array([total / cnt, np.float32(1) / cnt if cnt > 0 else np.float32(0)], dtype=np.float32)


XentCase = namedtuple("XentCase", "rows c ignore x t grad loss_rows out valid exact_loss")
# x float64 [rows, C]; t int64 [rows]; grad float64 [rows, C] (unscaled: softmax - onehot, 0 on ignored rows);
# loss_rows float64 [rows]; out numpy float32 [2]; exact_loss: loss_rows and out[0] are exact


def _xent_out(loss_rows: torch.Tensor, valid: int) -> np.ndarray:
    total = float(loss_rows.sum())
    assert total < FP32_EXACT and total == int(total)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.float32(total) / np.float32(valid)
    return np.array([mean, np.float32(1) / np.float32(valid) if valid else np.float32(0)], dtype=np.float32)


def xent_selection(rows: int, c: int, ignore: int, keep: int | None = None) -> XentCase:
    """Row r: hot class cycling over {0, 63, 64, 255, 256, C - 1} (where they
    exist) with value h = r % 4; target kind cycling with period 7 (coprime to
    every hot-class period) over: the hot class, another class, ignore_index,
    -100, -1, C, 255.  The last row is always valid with a target that is not
    the hot class (loss 256 + h): the ragged narrow block re-reads that row in
    its spare lanes, and counting it twice would change both sums.
    keep = k: only k rows spread over the range keep their target, the rest
    are ignored (the valid count is asserted to be k); keep = 0: all ignored."""
    r = torch.arange(rows)
    hots = sorted({v for v in (0, 63, 64, 255, 256, c - 1) if v < c})
    hot = torch.tensor(hots)[r % len(hots)]
    h = (r % 4).to(F64)
    kind = r % 7
    t = hot.clone()
    t[kind == 1] = ((hot + 1) % c)[kind == 1]
    t[kind == 2] = ignore
    t[kind == 3] = -100
    t[kind == 4] = -1
    t[kind == 5] = c
    t[kind == 6] = 255
    t[rows - 1] = (hot[rows - 1] + 1) % c
    if t[rows - 1] == ignore:
        t[rows - 1] = (hot[rows - 1] + 2) % c
    if keep is not None:
        if keep == 0:
            t[:] = ignore if 0 <= ignore < c else -100
        else:
            kinds = torch.arange(keep) % 2  # alternately the hot class and its neighbour
            at = torch.unique(torch.linspace(0, rows - 1, keep).round().to(I64))
            assert at.numel() == keep
            tt = torch.where(kinds == 0, hot[at], (hot[at] + 1) % c)
            tt[-1] = (hot[rows - 1] + 1) % c
            t[:] = -100
            t[at] = tt
            assert not bool((tt == ignore).any())
    x = torch.full((rows, c), OTHER, dtype=F64)
    x[r, hot] = h
    ok = xent_valid(t, c, ignore)
    grad = torch.zeros((rows, c), dtype=F64)
    grad[r, hot] = 1.0
    tc = t.clamp(0, c - 1)
    grad[r, tc] -= ok.to(F64)
    grad[~ok] = 0.0
    loss_rows = torch.where(ok & (t != hot), h - OTHER, torch.zeros_like(h))
    valid = int(ok.sum())
    assert keep is None or valid == keep
    assert c == 1 or rows == 1 or keep == 0 or bool((loss_rows > 0).any())
    assert bf16_exact(x) and bf16_exact(grad)
    return XentCase(rows, c, ignore, x, t, grad, loss_rows, _xent_out(loss_rows, valid), valid, True)


def xent_uniform(rows: int, c: int) -> XentCase:
    """Every class of row r holds h = r % 4 - 1; targets walk the classes, with
    every fifth row ignored (-100).  Gradient 1 / C - onehot(t) in float64."""
    assert c & (c - 1) == 0 and c <= 4096
    r = torch.arange(rows)
    t = (r * 37 + 1) % c
    t[r % 5 == 4] = -100
    t[rows - 1] = (rows * 37) % c
    x = ((r % 4) - 1).to(F64).view(rows, 1).expand(rows, c).contiguous()
    ok = xent_valid(t, c, -100)
    grad = torch.full((rows, c), 1.0 / c, dtype=F64)
    grad[r, t.clamp(0, c - 1)] -= ok.to(F64)
    grad[~ok] = 0.0
    assert f32_exact(grad)  # so the kernel's p - 1 is exact in fp32 and rounds once to bf16
    loss_rows = torch.where(ok, torch.full((rows,), float(np.log(np.float64(c))), dtype=F64), torch.zeros(rows, dtype=F64))
    valid = int(ok.sum())
    out = np.array([float(loss_rows.sum()) / valid, np.float32(1) / np.float32(valid)], dtype=np.float32)
    return XentCase(rows, c, -100, x, t, grad, loss_rows, out, valid, False)


@functools.lru_cache(maxsize=None)
def xent_case(family: str, rows: int, c: int, ignore: int = -100, keep: int | None = None) -> XentCase:
    return xent_uniform(rows, c) if family == "uniform" else xent_selection(rows, c, ignore, keep)


def xent_inside_ignore(c: int) -> int:
    """An ignore_index inside [0, C) that is none of the hot classes' neighbours' only choice."""
    return c // 2


XentLayout = namedtuple("XentLayout", "shape stride numel args")
# shape / stride of the logits tensor, elements of its storage, args = (hw, bstride, pstride, cstride)


def xent_layout(kind: str, rows: int, c: int, bchw=None) -> XentLayout:
    """How [rows, C] values sit in storage: 'dense', 'padded' (rows of C + 24),
    'cl' / 'nchw' ([B, C, H, W], rows = (b, h, w))."""
    if kind == "dense":
        return XentLayout((rows, c), (c, 1), rows * c, (rows, 0, c, 1))
    if kind == "padded":
        wd = c + PAD_COLS
        return XentLayout((rows, c), (wd, 1), rows * wd, (rows, 0, wd, 1))
    b, c4, h, w = bchw
    assert c4 == c and b * h * w == rows
    if kind == "cl":
        return XentLayout(bchw, (h * w * c, 1, w * c, c), rows * c, (h * w, h * w * c, c, 1))
    assert kind == "nchw"
    return XentLayout(bchw, (c * h * w, h * w, w, 1), rows * c, (h * w, c * h * w, 1, h * w))


def xent_offsets(lay: XentLayout, rows: int, c: int) -> torch.Tensor:
    """int64 [rows, C]: the storage offset of element (row, class), by the
    kernel header's formula base(row) + c * cstride."""
    hw, bs, ps, cs = lay.args
    r = torch.arange(rows).view(rows, 1)
    return (r // hw) * bs + (r % hw) * ps + torch.arange(c).view(1, c) * cs


def xent_store(lay: XentLayout, vals: torch.Tensor, dtype, fill: float) -> torch.Tensor:
    """Flat storage of lay.numel elements holding vals [rows, C] at the
    layout's offsets and `fill` everywhere else (the pad columns)."""
    rows, c = vals.shape
    off = xent_offsets(lay, rows, c).reshape(-1)
    assert off.unique().numel() == off.numel() and int(off.max()) < lay.numel
    s = torch.full((lay.numel,), fill, dtype=F64)
    s[off] = vals.reshape(-1)
    return s.to(dtype)


def xent_tensor(lay: XentLayout, store: torch.Tensor) -> torch.Tensor:
    return store.as_strided(lay.shape, lay.stride)


def xent_layout_cases():
    """(family, kind, rows, C, bchw, ignore) of every direct-call case."""
    out = []
    for (rows, c) in XENT_SHAPES:
        out.append(("selection", "dense", rows, c, None, xent_inside_ignore(c)))
    out.append(("selection", "dense", 257, 21, None, -100))
    out.append(("selection", "dense", 100, 1000, None, -100))
    for kind, shapes in XENT_MAPS.items():
        for bchw in shapes:
            b, c, h, w = bchw
            out.append(("selection", kind, b * h * w, c, bchw, 255 if c == 21 else xent_inside_ignore(c)))
    for rows, c in XENT_PADDED:
        out.append(("selection", "padded", rows, c, None, xent_inside_ignore(c)))
    for rows, c in XENT_UNIFORM:
        out.append(("uniform", "dense", rows, c, None, -100))
    out.append(("uniform", "padded", 70, 64, None, -100))
    return out


def xent_op_cases():
    """(kind, rows, C, bchw): one selection case per layout for the Python op."""
    return [("dense", 100, 1000, None), ("dense", 300, 21, None), ("padded", 257, 21, None), ("padded", 65, 65, None),
            ("cl", 70, 21, (2, 21, 5, 7)), ("cl", 18, 65, (2, 65, 3, 3)), ("nchw", 297, 64, (3, 64, 9, 11))]


# ---- SGD ------------------------------------------------------------------------------
SGD_CHUNK = 8192
SGD_MAX_SEG = 48
SGD_HP = {
    "plain": dict(lr=0.5, momentum=0.5, dampening=0.0, weight_decay=0.0, nesterov=False),
    "wd": dict(lr=0.5, momentum=0.5, dampening=0.0, weight_decay=0.25, nesterov=False),
    "damp": dict(lr=0.5, momentum=0.5, dampening=0.25, weight_decay=0.0, nesterov=False),
    "nesterov_wd": dict(lr=0.5, momentum=0.5, dampening=0.0, weight_decay=0.25, nesterov=True),
}
SGD_SIZES = {
    # nv = 257 vectors: a tail that crosses into the second of the four u iterations
    "sizes": (8, 2048, 2056, 8184, 8192, 8200, 3 * 8192 + 2056),
    "48x8": (8,) * 48,
    "big_ends": (2 * 8192 + 8,) + (8,) * 46 + (8192 + 2056,),
}
SGD_STEPS = 3


def sgd_blocks(sizes) -> list[int]:
    """first_blk as vgpu_sgd_bf16 builds it."""
    out, b = [], 0
    for n in sizes:
        out.append(b)
        b += (n + SGD_CHUNK - 1) // SGD_CHUNK
    return out + [b]


def sgd_covered(sizes, strict: bool = False) -> list[int]:
    """Elements of each segment that sgd_bf16_kernel's blocks update, as a CPU
    model of its segment search and tail: block b belongs to the last segment
    whose first block is <= b.  strict: the mistake of searching with `<`, which
    hands a segment's first block to the segment before it (where it lies past
    the end and does nothing)."""
    first = sgd_blocks(sizes)
    done = [0] * len(sizes)
    for b in range(first[-1]):
        seg = 0
        while seg + 1 < len(sizes) and (first[seg + 1] < b if strict else first[seg + 1] <= b):
            seg += 1
        base = (b - first[seg]) * SGD_CHUNK
        nv = (sizes[seg] - base) // 8  # negative past the end: no lane has i < nv
        done[seg] += 8 * max(0, min(nv, SGD_CHUNK // 8))
    return done


def sgd_step_ref(p, g, m, hp, first, exact=f32_exact):
    """One step of the header's formula in float64 on float64 tensors holding
    bf16 values.  Returns (p', m') unrounded; asserts that every intermediate
    is exact in float32 (so any fma contraction of the kernel's chain gives
    the same float32 number, which is then rounded once to bf16)."""
    lr, mom, damp, wd = hp["lr"], hp["momentum"], hp["dampening"], hp["weight_decay"]
    steps = []
    gg = g + wd * p
    steps += [wd * p, gg]
    if first:
        m2 = gg
    else:
        a, b = mom * m, (1.0 - damp) * gg
        m2 = a + b
        steps += [a, b, m2]
    if hp["nesterov"]:
        d = gg + mom * m2
        steps += [mom * m2, d]
    else:
        d = m2
    p2 = p - lr * d
    steps += [lr * d, p2]
    assert all(exact(s) for s in steps), "an intermediate of the SGD reference is not exact"
    return p2, m2


def sgd_run_ref(p0, gs, hp, m0=None, exact=f32_exact):
    """The states [(p, m)] after each gradient of gs, float64 holding bf16
    values: p and m rounded to bf16 once per step.  m0 None: the first step
    initialises the momentum from the gradient."""
    out = []
    p, m = p0.to(F64), None if m0 is None else m0.to(F64)
    for g in gs:
        p, m = sgd_step_ref(p, g.to(F64), m, hp, m is None, exact)
        p, m = p.to(BF).to(F64), m.to(BF).to(F64)
        out.append((p, m))
    return out


@functools.lru_cache(maxsize=None)
def sgd_case(name: str, steps: int = SGD_STEPS):
    """Per segment: p, m, and `steps` gradients, all non-zero integers |.| <= 4
    drawn independently (int64)."""
    g = E.gen(len(name) * 1000 + sum(SGD_SIZES[name]) % 997)
    segs = []
    for n in SGD_SIZES[name]:
        segs.append((E.nonzero_ints((n,), g, 4), E.nonzero_ints((n,), g, 4),
                     [E.nonzero_ints((n,), g, 4) for _ in range(steps)]))
    return segs


# the optimizer-class case: 50 eligible tensors (one channels-last) and one with numel % 8 != 0
SGD_CLASS_SHAPES = [(16, 8, 3, 3)] + [(8,), (2056,), (16, 24), (8200,)] + [(8 * (1 + i % 5),) for i in range(45)] + [(7, 5)]
SGD_CLASS_RUNS = {"plain": 3, "nesterov_wd": 1}  # steps for which every intermediate is bf16-exact too


@functools.lru_cache(maxsize=None)
def sgd_class_case(steps: int):
    g = E.gen(4242)
    return [(E.nonzero_ints(sh, g, 4), [E.nonzero_ints(sh, g, 4) for _ in range(steps)]) for sh in SGD_CLASS_SHAPES]


# ---- training max pool -----------------------------------------------------------------
POOL_THREADS = 256
POOL_MAX_BLOCKS = 256 * 16
# (k, stride, pad), (N, C, H, W)
POOL_SMALL = [
    ((3, 2, 1), (2, 16, 7, 9)),
    ((3, 1, 1), (1, 8, 5, 5)),
    ((2, 2, 0), (2, 24, 6, 7)),   # the last column lies in no window
    ((1, 1, 0), (1, 8, 3, 3)),
    ((5, 3, 2), (1, 8, 11, 13)),
    ((15, 1, 7), (1, 8, 16, 16)),
]
POOL_BIG = ((3, 2, 1), (2, 64, 512, 520))
POOL_KINDS = ("const", "ints", "nan")


def pool_grid(total: int) -> int:
    g = (total + POOL_THREADS - 1) // POOL_THREADS
    return max(1, min(g, POOL_MAX_BLOCKS))


def pool_totals(ksp, shape) -> tuple[int, int]:
    """(forward, backward) thread-item totals: N * OH * OW * C/8 and N * H * W * C/8."""
    k, s, p = ksp
    n, c, h, w = shape
    oh, ow = E.out_hw(h, w, k, s, p)
    return n * oh * ow * (c // 8), n * h * w * (c // 8)


def pool_inputs(ksp, shape, kind: str, seed: int = 0):
    """x float64 [N, H, W, C] (bf16 values, NaN / -inf for kind 'nan') and dy
    int64 [N, OH, OW, C], non-zero with |dy| <= 4."""
    k, s, p = ksp
    n, c, h, w = shape
    oh, ow = E.out_hw(h, w, k, s, p)
    g = E.gen(seed + 17 * k + h * w + c)
    if kind == "const":
        x = torch.randint(-3, 4, (n, 1, 1, c), generator=g).expand(n, h, w, c).to(F64).contiguous()
    else:
        x = torch.randint(-3, 4, (n, h, w, c), generator=g).to(F64)
    if kind == "nan":
        x[0, :, :, c - 1] = -float("inf")                 # one plane all -inf
        x[0, h // 2, w // 2, 0] = float("nan")            # a lone NaN
        x[0, 0, 0, 1] = float("nan")                      # at the corner
        x[n - 1, h - 1, w - 1, 1] = float("nan")
        if w > 1:
            x[0, h // 2, w // 2 - 1, 2] = float("nan")    # two in a row, three in an L:
            x[0, h // 2, w // 2, 2] = float("nan")        # windows holding several keep the last
        if h > 1:
            x[0, h // 2 - 1, w // 2, 2] = float("nan")
        x[0, 0, 0, 3] = -float("inf")                     # -inf among numbers
    dy = E.nonzero_ints((n, oh, ow, c), g, 4)
    assert k * k * 4 < FP32_EXACT
    return x, dy


def pool_loop_ref(x: torch.Tensor, dy: torch.Tensor, ksp, strict: bool = True):
    """The kernel header's rule as a plain loop over the taps in (kh, kw)
    order: the first tap inside the image starts the window, a later one wins
    when it is strictly greater or a NaN, padding is skipped.  Returns y
    float64 [N, OH, OW, C], tap uint8 [N, OH, OW, C] and dx float64 [N, H, W, C]
    = the sum of dy over the windows whose tap is that pixel.
    strict=False: the mistake of comparing with >= (the last maximum wins)."""
    k, s, p = ksp
    n, h, w, c = x.shape
    oh, ow = E.out_hw(h, w, k, s, p)
    xa = x.numpy()
    y = np.full((n, oh, ow, c), -np.inf)
    tap = np.full((n, oh, ow, c), 0xFF, dtype=np.uint8)
    ohs, ows = np.arange(oh), np.arange(ow)
    for dh in range(k):
        ih = ohs * s - p + dh
        vh = (ih >= 0) & (ih < h)
        for dw in range(k):
            iw = ows * s - p + dw
            vw = (iw >= 0) & (iw < w)
            e = xa[:, np.clip(ih, 0, h - 1)][:, :, np.clip(iw, 0, w - 1)]
            inside = (vh[:, None] & vw[None, :])[None, :, :, None]
            with np.errstate(invalid="ignore"):
                take = inside & ((e > y if strict else e >= y) | np.isnan(e) | (tap == 0xFF))
            y = np.where(take, e, y)
            tap = np.where(take, np.uint8(dh * k + dw), tap)
    assert not (tap == 0xFF).any()  # pad <= k / 2: every window holds a pixel
    dx = np.zeros((n, h, w, c))
    dya = dy.numpy().astype(np.float64)
    ni, oi, oj, ci = np.indices((n, oh, ow, c))
    ih = oi * s - p + tap // k
    iw = oj * s - p + tap % k
    assert (ih >= 0).all() and (ih < h).all() and (iw >= 0).all() and (iw < w).all()
    np.add.at(dx, (ni, ih, iw, ci), dya)
    return torch.from_numpy(y), torch.from_numpy(tap), torch.from_numpy(dx)


def pool_torch_ref(x: torch.Tensor, dy: torch.Tensor, ksp, dtype=F64):
    """The same three results from F.max_pool2d(return_indices=True) and its
    backward (no NaN in x).  x [N, H, W, C], dy [N, OH, OW, C]."""
    k, s, p = ksp
    n, h, w, c = x.shape
    xt = x.permute(0, 3, 1, 2).to(dtype).requires_grad_()
    y, ind = torch.nn.functional.max_pool2d(xt, k, s, p, return_indices=True)
    (dx,) = torch.autograd.grad(y, xt, dy.permute(0, 3, 1, 2).to(dtype))
    oh, ow = y.shape[2:]
    ih, iw = ind // w, ind % w
    dh = ih - (torch.arange(oh).view(1, 1, oh, 1) * s - p)
    dw = iw - (torch.arange(ow).view(1, 1, 1, ow) * s - p)
    assert bool(((dh >= 0) & (dh < k) & (dw >= 0) & (dw < k)).all())
    tap = (dh * k + dw).to(torch.uint8)
    return y.detach().permute(0, 2, 3, 1), tap.permute(0, 2, 3, 1), dx.permute(0, 2, 3, 1)


@functools.lru_cache(maxsize=1)
def pool_big_case():
    """The grid-stride case: integers in [-3, 3], reference from torch ops in
    float32 (exact for these values; the float64 planes would be 270 MB)."""
    ksp, shape = POOL_BIG
    x, dy = pool_inputs(ksp, shape, "ints")
    y, tap, dx = pool_torch_ref(x, dy, ksp, F32)
    return x.to(BF), dy.to(BF), y.to(BF).contiguous(), tap.contiguous(), dx.to(BF).contiguous()


# ---- bilinear resize -------------------------------------------------------------------
# (N, (IH, IW), (OH, OW))
RESIZE_CASES = [
    (1, (5, 3), (10, 12)),
    (1, (3, 3), (48, 48)),
    (2, (8, 6), (4, 3)),
    (1, (1, 1), (4, 4)),
    (2, (1, 4), (2, 4)),
    (2, (24, 24), (48, 48)),  # P = 4608: 18 blocks of 256 pixels
    (1, (5, 3), (20, 3)),     # P = 60: one ragged block, and j = 2, 0
]
RESIZE_C_SCALAR = (1, 21, 30)
RESIZE_C_VECTOR = (8, 24)
RESIZE_J = (-1, 0, 1, 2, 4)


def resize_src(out: int, inp: int):
    """(i0, i1, l0, l1) float64 / int64 [out] by PyTorch's rule: src =
    max(scale * (o + 0.5) - 0.5, 0), i1 clamped to the last pixel.  Asserts the
    exactness the comparison rests on."""
    j = {inp * 2 ** j if j >= 0 else inp // 2 ** -j: j for j in RESIZE_J if j >= 0 or inp % 2 ** -j == 0}
    assert out in j, (inp, out)
    scale = inp / out
    o = torch.arange(out, dtype=F64)
    raw = scale * (o + 0.5) - 0.5
    src = raw.clamp_min(0.0)
    i0 = src.floor().to(I64)
    # the kernel's `i0 > in - 1` clamp never fires: src < in - 0.5 for every o < out
    assert int(i0.max()) <= inp - 1
    i1 = torch.where(i0 < inp - 1, i0 + 1, i0)
    l1 = src - i0.to(F64)
    l0 = 1.0 - l1
    for lam in (l0, l1):
        assert bool(((lam * 64) == (lam * 64).round()).all()) and bool(((lam >= 0) & (lam <= 1)).all())
    return i0, i1, l0, l1


def resize_ref(x: torch.Tensor, size) -> torch.Tensor:
    """x float64 [N, IH, IW, C] -> float64 [N, OH, OW, C], the kernel's
    expression h0 * (w0 * x00 + w1 * x01) + h1 * (w0 * x10 + w1 * x11)."""
    n, ih, iw, c = x.shape
    assert float(x.abs().max()) <= 100 and bool((x == x.round()).all())
    h0, h1, hl0, hl1 = resize_src(size[0], ih)
    w0, w1, wl0, wl1 = resize_src(size[1], iw)
    wl0, wl1 = wl0.view(1, 1, -1, 1), wl1.view(1, 1, -1, 1)
    hl0, hl1 = hl0.view(1, -1, 1, 1), hl1.view(1, -1, 1, 1)
    top = wl0 * x[:, h0][:, :, w0] + wl1 * x[:, h0][:, :, w1]
    bot = wl0 * x[:, h1][:, :, w0] + wl1 * x[:, h1][:, :, w1]
    y = hl0 * top + hl1 * bot
    for t in (wl0 * x[:, h0][:, :, w0], top, bot, hl0 * top, hl1 * bot, y):
        assert f32_exact(t)
    return y


@functools.lru_cache(maxsize=None)
def resize_case(n: int, in_hw, out_hw, c: int, const: bool = False):
    """x int64 [N, IH, IW, C] in [-100, 100] (const: image i holds one value,
    different per image) and the reference rounded once to bf16."""
    g = E.gen(n * 7 + in_hw[0] * 31 + out_hw[1] * 3 + c)
    if const:
        x = torch.tensor([7, -5, 3, 100][:n]).view(n, 1, 1, 1).expand(n, *in_hw, c).contiguous()
    else:
        x = torch.randint(-100, 101, (n, *in_hw, c), generator=g)
    return x, resize_ref(x.to(F64), out_hw).to(BF)
