"""Numerics of native/kernels/lstm.hip: carried state (the *_window entry
points), single steps into saturation, window-against-one-call bit exactness,
the two-layer wavefront against the layer-by-layer kernels on identical inputs,
and 1024-step runs and dense-loss gradients against an fp64 reference.

Reference: a plain fp64 step loop (`ref_layer` / `ref_stack`), itself checked
against fp64 torch.nn.LSTM on the CPU (C1).  "exact" is that loop on the
bf16-valued weights and inputs; "emulated" is the same loop with the two
roundings the design makes on the recurrence (Xp to bf16, h_t to bf16 at every
hand-off).  max|emulated - exact| is the design's floor; the long-sequence
tests bound the kernels by 3 x that floor, computed here and never taken from
the kernels.

Every buffer a kernel writes through a direct library call is allocated with
16 further rows of 0xFF bytes (NaN in bf16 and fp32), and those rows must be
untouched afterwards: the dead rows of a partial 16-row block store nothing.

Which test fails for which mistake (argued from lstm.hip):
  * c0 dropped (cells start at 0 in a window): G1 cells/c_state at first = 0,
    and G2 cells from the second window on.
  * has_prev ignored (c_{t-1} = 0 at a window's first step): G3 has_prev = 1
    (the f-gate block of dgates), and G4 dgates at t = 1, 8, 16, 25.
  * has_prev always read: G3 has_prev = 0, where the slot before `cells` holds
    1e30.
  * the count published before the step's stores (a role's fence dropped, or
    the count one too high): the reader may load the 0xFF fill of y1t / xp2 /
    dgates2 / dy1 instead of the step's data -> G5's torch.equal against the
    layer-by-layer kernels.  A count one too high names a step not yet computed
    and is seen at once; a dropped fence is seen only when the hardware really
    reorders, which a test cannot force.
  * pub_step off by one in its tail term (`done + 2 == total`, `done == total`):
    the steps after the last multiple of 8 are never published, the reader's
    wait gives up, the error flag is set and the outputs differ -> G5 at
    T = 1, 7, 9, 33 (T = 8, and the suite's earlier T = 40, 48, 64, end on a
    multiple of 8 and cannot see it).  An off-by-one in the `% kPubEvery` term
    moves when counts are published but still ends at T: no wrong result, and
    no test fails.
"""
import functools

import pytest
import torch

H = 128
BF = torch.bfloat16
F64 = torch.float64


# ---- reference (CPU, fp64) --------------------------------------------------------------

def _bf(t):
    """Round to bf16, keep fp64."""
    return t.to(BF).to(F64)


def ref_layer(xp, w_hh, h0=None, c0=None, round_h=False):
    """One layer's recurrence.  xp [T, B, 4H] (biases folded in), gate order
    i, f, g, o.  Returns y [T, B, H], activated gates [T, B, 4H], cells [T, B, H]."""
    T, B, _ = xp.shape
    h = torch.zeros(B, H, dtype=F64) if h0 is None else h0
    c = torch.zeros(B, H, dtype=F64) if c0 is None else c0
    wt = w_hh.t()
    ys, gs, cs = [], [], []
    for t in range(T):
        i, f, g, o = (xp[t] + h @ wt).chunk(4, dim=1)
        i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
        c = f * c + i * g
        h = o * torch.tanh(c)
        if round_h:
            h = _bf(h)
        ys.append(h), gs.append(torch.cat([i, f, g, o], dim=1)), cs.append(c)
    return torch.stack(ys), torch.stack(gs), torch.stack(cs)


def ref_stack(x, layers, emulate=False):
    """x [B, T, E]; layers: (w_ih, w_hh, b_ih, b_hh) each.  Zero initial state.
    emulate: Xp and every h_t rounded to bf16.  Returns (y, gates, cells) per layer."""
    inp = x.transpose(0, 1)
    out = []
    for w_ih, w_hh, b_ih, b_hh in layers:
        xp = inp @ w_ih.t() + b_ih + b_hh
        if emulate:
            xp = _bf(xp)
        out.append(ref_layer(xp, w_hh, round_h=emulate))
        inp = out[-1][0]
    return out


def ref_step_backward(gates, c, c_prev, dy, dh_in, dc_in, w_hh):
    """One step of the backward through time (lstm.hip, backward kernel header).
    Returns dgates (pre-activation) [B, 4H], dh_out [B, H], dc_out [B, H]."""
    i, f, g, o = gates.chunk(4, dim=1)
    dh = dy + dh_in
    tc = torch.tanh(c)
    dc = dh * o * (1 - tc * tc) + dc_in
    dgates = torch.cat([dc * g * i * (1 - i), dc * c_prev * f * (1 - f), dc * i * (1 - g * g),
                        dh * tc * o * (1 - o)], dim=1)
    return dgates, dgates @ w_hh, dc * f


def _params(layers, e, seed):
    """Default nn.LSTM init x 2, rounded to bf16 (the scale of tests/test_gpu_kernels.py)."""
    torch.manual_seed(seed)
    lstm = torch.nn.LSTM(e, H, num_layers=layers, batch_first=True)
    return [(p.detach() * 2.0).to(BF) for p in lstm.parameters()]


@functools.lru_cache(maxsize=None)
def _long_case(layers, b, t, e=64):
    """Inputs of G6 / C2, their exact output (last layer, [T, B, H]) and the floor."""
    with torch.random.fork_rng(devices=[]):
        params = _params(layers, e, seed=6)
        x = (torch.randn(b, t, e) * 0.5).to(BF)
    p64 = [p.to(F64) for p in params]
    stack = [tuple(p64[4 * k:4 * k + 4]) for k in range(layers)]
    with torch.no_grad():
        exact = ref_stack(x.to(F64), stack)[-1][0]
        emulated = ref_stack(x.to(F64), stack, emulate=True)[-1][0]
    return {"x": x, "params": params, "exact": exact, "floor": (emulated - exact).abs().max().item()}


@functools.lru_cache(maxsize=None)
def _grad_case(b, t, e=64):
    """Inputs of G7 and the fp64 torch.nn.LSTM gradients of sum_t y_t . head_t."""
    with torch.random.fork_rng(devices=[]):
        params = _params(2, e, seed=7)
        x = (torch.randn(b, t, e) * 0.5).to(BF)
        head = torch.randn(t, H)
    ref = torch.nn.LSTM(e, H, num_layers=2, batch_first=True).to(F64)
    with torch.no_grad():
        for p, q in zip(ref.parameters(), params):
            p.copy_(q)
    xr = x.to(F64).requires_grad_(True)
    (ref(xr)[0] * head.to(F64)).sum().backward()
    grads = {n: p.grad for n, p in ref.named_parameters()}
    grads["x"] = xr.grad
    return {"x": x, "params": params, "head": head, "grads": grads}


LONG = [(2, 20, 1024), (1, 37, 33)]  # (layers, B, T) of G6


# ---- C1 / C2 (CPU) ----------------------------------------------------------------------

def test_reference_matches_fp64_nn_lstm():
    """C1: the exact helper, and the one-step backward, against fp64 torch autograd."""
    torch.manual_seed(0)
    b, t, e = 3, 9, 20
    ref = torch.nn.LSTM(e, H, num_layers=2, batch_first=True).to(F64)
    x = torch.randn(b, t, e, dtype=F64)
    head = torch.randn(b, t, H, dtype=F64)
    xr = x.clone().requires_grad_(True)
    want = ref(xr)[0]
    (want * head).sum().backward()
    mine = [p.detach().clone().requires_grad_(True) for p in ref.parameters()]
    xm = x.clone().requires_grad_(True)
    got = ref_stack(xm, [tuple(mine[0:4]), tuple(mine[4:8])])[-1][0].transpose(0, 1)
    (got * head).sum().backward()
    assert (got - want).abs().max().item() <= 1e-10
    for (name, p), q in zip(ref.named_parameters(), mine):
        assert (q.grad - p.grad).abs().max().item() <= 1e-10, name
    assert (xm.grad - xr.grad).abs().max().item() <= 1e-10

    # one exact step with a carried state, against autograd of that step
    w_hh = ref.weight_hh_l0.detach()
    xp = (torch.randn(1, b, 4 * H, dtype=F64) * 2).requires_grad_(True)
    h0 = (torch.rand(b, H, dtype=F64) * 2 - 1).requires_grad_(True)
    c0 = (torch.rand(b, H, dtype=F64) * 8 - 4).requires_grad_(True)
    y, gates, cells = ref_layer(xp, w_hh, h0, c0)
    dy, dh_in, dc_in = (torch.randn(b, H, dtype=F64) for _ in range(3))
    dxp, dh0, dc0 = torch.autograd.grad((y[0], cells[0]), (xp, h0, c0), grad_outputs=(dy + dh_in, dc_in))
    dgates, dh_out, dc_out = ref_step_backward(gates[0].detach(), cells[0].detach(), c0.detach(), dy, dh_in, dc_in,
                                               w_hh)
    assert (dgates - dxp[0]).abs().max().item() <= 1e-10
    assert (dh_out - dh0).abs().max().item() <= 1e-10
    assert (dc_out - dc0).abs().max().item() <= 1e-10


@pytest.mark.parametrize("layers,b,t", LONG)
def test_long_inputs_have_a_small_floor_and_large_h(layers, b, t):
    """C2: conditions on G6's inputs, so that its bound 3 x floor stays below
    1.2e-2 and |h| is large enough for that bound to mean something."""
    case = _long_case(layers, b, t)
    hmax = case["exact"].abs().max().item()
    print(f"floor {case['floor']:.3e}  max|h| {hmax:.3f}")
    assert case["floor"] <= 4e-3
    assert hmax >= 0.3


# ---- GPU helpers ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib(gpu_build):
    from vgpu.native import load_kernels
    return load_kernels()


class Guarded:
    """rows x width elements for a kernel to write, then 16 sentinel rows; all
    bytes start as 0xFF (NaN in bf16 and fp32, so an element never written shows)."""

    def __init__(self, rows, width, dtype):
        n = rows * width * torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full((n // rows * (rows + 16),), 0xFF, dtype=torch.uint8, device="cuda")
        self.t = self.raw[:n].view(dtype).view(rows, width)
        self.tail = self.raw[n:]

    def ptr(self, off=0):
        return self.t.data_ptr() + off * self.t.element_size()

    def cpu(self):
        return self.t.cpu()


def _intact(*bufs):
    return all(bool((g.tail == 0xFF).all()) for g in bufs)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _weight(gen, rows=4 * H):
    """bf16 [rows, H], uniform in +-2/sqrt(H): default init x 2."""
    return ((torch.rand(rows, H, generator=gen) * 2 - 1) * (2.0 / H ** 0.5)).to(BF)


def _half_ulp(got, want, extra, what):
    """|got - want| <= 2^-8 |want| + extra (half a bf16 ulp of want, plus `extra`)."""
    got, want = got.to(F64), want.to(F64)
    assert bool(torch.isfinite(got).all()), what
    err = (got - want).abs()
    bound = want.abs() * 2.0 ** -8 + extra
    print(f"{what}: max err {err.max().item():.3e}, max err/bound {(err / bound).max().item():.3f}")
    assert bool((err <= bound).all()), (what, err.max().item())


def _dot_bound(a_abs, w_abs_t, k):
    """fp32 dot-product error bound 2 k 2^-24 sum_k |a_k w_k|."""
    return 2.0 * k * 2.0 ** -24 * (a_abs.to(F64) @ w_abs_t.to(F64))


# ---- G1: one forward step with carried state, into saturation --------------------------------

SAT = (200.0, -200.0, 30.0, -30.0, 0.0, None, None, None)


@pytest.mark.gpu
@pytest.mark.parametrize("b", [1, 16, 37])
def test_forward_step_with_carried_state(lib, b):
    """G1: vgpu_lstm_recurrence_window, T = 1, from (h0, c0) and from NaN-filled
    state with first = 1, pre-activations forced to +-200, +-30 and 0."""
    gen = torch.Generator().manual_seed(100 + b)
    w_hh = _weight(gen)
    h0 = (torch.rand(b, H, generator=gen) * 2 - 1).to(BF)
    c0 = torch.rand(b, H, generator=gen) * 8 - 4
    xp = torch.randn(1, b, 4 * H, generator=gen) * 2
    for q in range(4):          # groups of 8 units; the gates of one unit get different values
        for j in range(16):
            v = SAT[(j + 3 * q) % 8]
            if v is not None:
                xp[..., q * H + 8 * j:q * H + 8 * j + 8] = v
    xp = xp.to(BF)
    xp_d, w_d = xp.cuda(), w_hh.cuda()
    for first in (0, 1):
        hs, cs = Guarded(b, H, BF), Guarded(b, H, torch.float32)
        if not first:
            hs.t.copy_(h0), cs.t.copy_(c0)
        y, gates, cells = Guarded(b, H, BF), Guarded(b, 4 * H, BF), Guarded(b, H, torch.float32)
        rc = lib.vgpu_lstm_recurrence_window(xp_d.data_ptr(), w_d.data_ptr(), y.ptr(), H, H, hs.ptr(), cs.ptr(), first,
                                             gates.ptr(), cells.ptr(), b, 1, H, None, _stream())
        assert rc == 0
        torch.cuda.synchronize()
        want_y, want_g, want_c = ref_layer(xp.to(F64), w_hh.to(F64), None if first else h0.to(F64),
                                           None if first else c0.to(F64))
        got_c = cells.cpu()
        assert bool(torch.isfinite(got_c).all())
        err = (got_c.to(F64) - want_c[0]).abs().max().item()
        print(f"first={first} cells: max err {err:.3e}")
        assert err <= 1e-4
        assert torch.equal(cs.cpu(), got_c)
        _half_ulp(y.cpu(), want_y[0], 1e-5, f"first={first} y")
        _half_ulp(hs.cpu(), want_y[0], 1e-5, f"first={first} h_state")
        _half_ulp(gates.cpu(), want_g[0], 1e-5, f"first={first} gates")
        assert _intact(hs, cs, y, gates, cells)


# ---- G2 / G4: windows are bit-exact with one call ------------------------------------------------

WINDOWS = (1, 7, 8, 9, 2)


@pytest.fixture(scope="module")
def saved(lib):
    """G2's one-call forward (B = 37, T = 27), kept for G4."""
    b, t = 37, sum(WINDOWS)
    gen = torch.Generator().manual_seed(2)
    w = _weight(gen).cuda()
    xp = torch.randn(t, b, 4 * H, generator=gen).to(BF).cuda()
    y, gates, cells = Guarded(b, t * H, BF), Guarded(t * b, 4 * H, BF), Guarded(t * b, H, torch.float32)
    assert lib.vgpu_lstm_forward_train(xp.data_ptr(), w.data_ptr(), y.ptr(), gates.ptr(), cells.ptr(), b, t, H,
                                       _stream()) == 0
    torch.cuda.synchronize()
    for g in (y, gates, cells):
        assert bool(torch.isfinite(g.t).all())
    assert _intact(y, gates, cells)
    return {"b": b, "t": t, "w": w, "xp": xp, "y": y.t.view(b, t, H), "gates": gates.t, "cells": cells.t}


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["batch_major", "timestep_major"])
def test_forward_windows_bit_exact(lib, saved, layout):
    """G2: windows of 1, 7, 8, 9, 2 steps against vgpu_lstm_forward_train in one call."""
    b, t, w, xp = saved["b"], saved["t"], saved["w"], saved["xp"]
    if layout == "batch_major":
        y, ys_row, ys_t = Guarded(b, t * H, BF), t * H, H
    else:
        y, ys_row, ys_t = Guarded(t * b, H, BF), H, b * H
    gates, cells = Guarded(t * b, 4 * H, BF), Guarded(t * b, H, torch.float32)
    hs, cs = Guarded(b, H, BF), Guarded(b, H, torch.float32)
    t0 = 0
    for n in WINDOWS:
        rc = lib.vgpu_lstm_recurrence_window(xp.data_ptr() + t0 * b * 4 * H * 2, w.data_ptr(), y.ptr(t0 * ys_t), ys_row,
                                             ys_t, hs.ptr(), cs.ptr(), int(t0 == 0), gates.ptr(t0 * b * 4 * H),
                                             cells.ptr(t0 * b * H), b, n, H, None, _stream())
        assert rc == 0
        t0 += n
    torch.cuda.synchronize()
    got_y = y.t.view(b, t, H) if layout == "batch_major" else y.t.view(t, b, H).transpose(0, 1)
    assert torch.equal(got_y, saved["y"])
    assert torch.equal(gates.t, saved["gates"])
    assert torch.equal(cells.t, saved["cells"])
    assert torch.equal(cs.t, saved["cells"].view(t, b, H)[-1])
    assert torch.equal(hs.t, saved["y"][:, -1])
    assert _intact(y, gates, cells, hs, cs)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["batch_major", "timestep_major"])
def test_backward_windows_bit_exact(lib, saved, layout):
    """G4: windows of 2, 9, 8, 7, 1 steps, newest first, against vgpu_lstm_backward in one call."""
    b, t, w = saved["b"], saved["t"], saved["w"]
    gates, cells = saved["gates"], saved["cells"]
    gen = torch.Generator().manual_seed(4)
    dy = torch.randn(b, t, H, generator=gen).to(BF).cuda()
    one = Guarded(t * b, 4 * H, BF)
    assert lib.vgpu_lstm_backward(gates.data_ptr(), cells.data_ptr(), dy.data_ptr(), w.data_ptr(), one.ptr(), b, t, H,
                                  _stream()) == 0
    if layout == "batch_major":
        dyw, ds_row, ds_t = dy, t * H, H
    else:
        dyw, ds_row, ds_t = dy.transpose(0, 1).contiguous(), H, b * H
    win = Guarded(t * b, 4 * H, BF)
    dh, dc = Guarded(b, H, torch.float32), Guarded(b, H, torch.float32)
    dh.t.zero_(), dc.t.zero_()
    t1 = t
    for n in reversed(WINDOWS):  # newest window first
        t0 = t1 - n
        rc = lib.vgpu_lstm_backward_window(gates.data_ptr() + t0 * b * 4 * H * 2, cells.data_ptr() + t0 * b * H * 4,
                                           dyw.data_ptr() + t0 * ds_t * 2, ds_row, ds_t, w.data_ptr(),
                                           win.ptr(t0 * b * 4 * H), dh.ptr(), dc.ptr(), int(t0 > 0), b, n, H, _stream())
        assert rc == 0
        t1 = t0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(one.t).all())
    assert torch.equal(win.t, one.t)
    assert bool(torch.isfinite(dh.t).all()) and bool(torch.isfinite(dc.t).all())
    assert _intact(one, win, dh, dc)


# ---- G3: one backward step with carried gradients ------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("with_dy", [False, True])
@pytest.mark.parametrize("has_prev", [0, 1])
@pytest.mark.parametrize("b", [1, 16, 37])
def test_backward_step_with_carried_gradients(lib, b, has_prev, with_dy):
    """G3: vgpu_lstm_backward_window, T = 1, carried (dh, dc), saturated gates."""
    gen = torch.Generator().manual_seed(300 + b)
    w_hh = _weight(gen)
    gates = torch.rand(b, 4 * H, generator=gen)
    gates[:, 2 * H:3 * H] = gates[:, 2 * H:3 * H] * 2 - 1  # g in (-1, 1)
    for q in range(4):                                     # saturated groups of 8 units, staggered by gate
        lo = -1.0 if q == 2 else 0.0
        gates[:, q * H + 8 * q:q * H + 8 * q + 8] = lo
        gates[:, q * H + 8 * q + 64:q * H + 8 * q + 72] = 1.0
    gates = gates.to(BF)
    c = torch.rand(b, H, generator=gen) * 12 - 6
    c_prev = torch.rand(b, H, generator=gen) * 12 - 6
    dy = torch.randn(b, H, generator=gen).to(BF)
    dh_in, dc_in = torch.randn(b, H, generator=gen), torch.randn(b, H, generator=gen)
    # the slot before `cells` holds c_{t-1}, or something that must not be read
    cbuf = torch.stack([c_prev if has_prev else torch.full((b, H), 1e30), c]).cuda()
    g_d, w_d, dy_d = gates.cuda(), w_hh.cuda(), dy.cuda()
    dgates, dh, dc = Guarded(b, 4 * H, BF), Guarded(b, H, torch.float32), Guarded(b, H, torch.float32)
    dh.t.copy_(dh_in), dc.t.copy_(dc_in)
    rc = lib.vgpu_lstm_backward_window(g_d.data_ptr(), cbuf[1].data_ptr(), dy_d.data_ptr() if with_dy else None, H, H,
                                       w_d.data_ptr(), dgates.ptr(), dh.ptr(), dc.ptr(), has_prev, b, 1, H, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    zero = torch.zeros(b, H, dtype=F64)
    want_dg, _, want_dc = ref_step_backward(gates.to(F64), c.to(F64), c_prev.to(F64) if has_prev else zero,
                                            dy.to(F64) if with_dy else zero, dh_in.to(F64), dc_in.to(F64),
                                            w_hh.to(F64))
    got_dg, got_dh, got_dc = dgates.cpu(), dh.cpu(), dc.cpu()
    _half_ulp(got_dg, want_dg, 1e-4, "dgates")
    assert bool(torch.isfinite(got_dc).all()) and bool(torch.isfinite(got_dh).all())
    err = (got_dc.to(F64) - want_dc).abs()
    bound = 1e-5 * want_dc.abs() + 1e-6
    print(f"dc_out: max err {err.max().item():.3e}, max err/bound {(err / bound).max().item():.3f}")
    assert bool((err <= bound).all())
    # dh_out = dgates . W_hh on the kernel's own (bf16) dgates
    err = (got_dh.to(F64) - got_dg.to(F64) @ w_hh.to(F64)).abs()
    bound = _dot_bound(got_dg.abs(), w_hh.abs(), 4 * H)
    print(f"dh_out: max err {err.max().item():.3e}, max err/bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert bool((err <= bound).all())
    assert _intact(dgates, dh, dc)


# ---- G5: the wavefront against layer by layer on identical inputs --------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("b,t", [(1, 1), (16, 7), (17, 8), (37, 9), (129, 33)])
def test_wavefront_matches_layer_by_layer(lib, b, t):
    """G5: vgpu_lstm2_forward / vgpu_lstm2_backward (training mode) against the
    one-layer kernels; T below, at and above kPubEvery = 8 and with a ragged tail,
    B = 129: a second placement group."""
    e = 64
    gen = torch.Generator().manual_seed(500 + b)
    w_ih1 = ((torch.rand(4 * H, e, generator=gen) * 2 - 1) * (2.0 / H ** 0.5)).to(BF)
    whh1, wih2, whh2 = _weight(gen), _weight(gen), _weight(gen)
    b1 = (torch.rand(4 * H, generator=gen) * 2 - 1) * (4.0 / H ** 0.5)  # b_ih + b_hh, each default init x 2
    b2 = ((torch.rand(4 * H, generator=gen) * 2 - 1) * (4.0 / H ** 0.5)).to(BF)
    x = (torch.randn(t, b, e, generator=gen) * 0.5).to(BF)
    xp1 = (x.to(F64) @ w_ih1.to(F64).t() + b1.to(F64)).to(BF).cuda()
    whh1_d, wih2_d, whh2_d, b2_d = whh1.cuda(), wih2.cuda(), whh2.cuda(), b2.cuda()
    nblk = (b + 15) // 16
    flags = torch.full((2 * nblk + 1,), -1, dtype=torch.int32, device="cuda")
    st = _stream()

    def act(width=H, dtype=BF):
        return Guarded(t * b, width, dtype)

    # forward, training mode
    y1t, xp2, y2t, hlast = act(), act(4 * H), act(), Guarded(b, H, BF)
    g1, g2, c1, c2 = act(4 * H), act(4 * H), act(H, torch.float32), act(H, torch.float32)
    rc = lib.vgpu_lstm2_forward(xp1.data_ptr(), whh1_d.data_ptr(), wih2_d.data_ptr(), b2_d.data_ptr(),
                                whh2_d.data_ptr(), y1t.ptr(), xp2.ptr(), flags.data_ptr(), hlast.ptr(), y2t.ptr(),
                                g1.ptr(), g2.ptr(), c1.ptr(), c2.ptr(), b, t, H, st)
    assert rc == 0
    torch.cuda.synchronize()
    assert lib.vgpu_lstm2_flags_error(flags.data_ptr(), b) == 0
    assert _intact(y1t, xp2, y2t, hlast, g1, g2, c1, c2)

    def layered(xp, whh):
        y, g, c = Guarded(b, t * H, BF), act(4 * H), act(H, torch.float32)
        assert lib.vgpu_lstm_forward_train(xp, whh.data_ptr(), y.ptr(), g.ptr(), c.ptr(), b, t, H, st) == 0
        torch.cuda.synchronize()
        assert bool(torch.isfinite(y.t).all()) and bool(torch.isfinite(g.t).all()) and bool(torch.isfinite(c.t).all())
        assert _intact(y, g, c)
        return y.t.view(b, t, H).transpose(0, 1).reshape(t * b, H), g.t, c.t

    ly, lg, lc = layered(xp1.data_ptr(), whh1_d)
    assert torch.equal(y1t.t, ly) and torch.equal(g1.t, lg) and torch.equal(c1.t, lc)
    y1_64 = y1t.cpu().to(F64)
    want = y1_64 @ wih2.to(F64).t() + b2.to(F64)
    _half_ulp(xp2.cpu(), want, _dot_bound(y1_64.abs(), wih2.abs().t(), H) + 2.0 * H * 2.0 ** -24 * b2.to(F64).abs(),
              "xp2")
    ly, lg, lc = layered(xp2.ptr(), whh2_d)
    assert torch.equal(y2t.t, ly) and torch.equal(g2.t, lg) and torch.equal(c2.t, lc)
    assert torch.equal(hlast.t, y2t.t.view(t, b, H)[-1])

    # backward on that saved state, dense dy2 [B, T, H]
    dy2 = torch.randn(b, t, H, generator=gen).to(BF).cuda()
    dg1, dg2, dy1 = act(4 * H), act(4 * H), act()
    rc = lib.vgpu_lstm2_backward(g1.ptr(), c1.ptr(), g2.ptr(), c2.ptr(), dy2.data_ptr(), whh1_d.data_ptr(),
                                 whh2_d.data_ptr(), wih2_d.data_ptr(), dg1.ptr(), dg2.ptr(), dy1.ptr(),
                                 flags.data_ptr(), b, t, H, st)
    assert rc == 0
    torch.cuda.synchronize()
    assert lib.vgpu_lstm2_flags_error(flags.data_ptr(), b) == 0
    assert _intact(dg1, dg2, dy1)

    def layered_bwd(g, c, dy, whh):
        dg = act(4 * H)
        assert lib.vgpu_lstm_backward(g.ptr(), c.ptr(), dy.data_ptr(), whh.data_ptr(), dg.ptr(), b, t, H, st) == 0
        torch.cuda.synchronize()
        assert bool(torch.isfinite(dg.t).all()) and _intact(dg)
        return dg.t

    assert torch.equal(dg2.t, layered_bwd(g2, c2, dy2, whh2_d))
    dg2_64 = dg2.cpu().to(F64)
    _half_ulp(dy1.cpu(), dg2_64 @ wih2.to(F64), _dot_bound(dg2_64.abs(), wih2.abs(), 4 * H), "dy1")
    dy1_bm = dy1.t.view(t, b, H).transpose(0, 1).contiguous()
    assert torch.equal(dg1.t, layered_bwd(g1, c1, dy1_bm, whh1_d))


# ---- G6 / G7: long sequences through vgpu.ops.lstm -----------------------------------------------

def _gpu_lstm(params, e, layers):
    mod = torch.nn.LSTM(e, H, num_layers=layers, batch_first=True).to(BF).cuda()
    with torch.no_grad():
        for p, q in zip(mod.parameters(), params):
            p.copy_(q)
    return mod


def _check_long(fused, layers, b, t):
    case = _long_case(layers, b, t)
    mod, x = _gpu_lstm(case["params"], 64, layers), case["x"].cuda()
    exact, floor = case["exact"], case["floor"]
    with torch.no_grad():
        y = fused.lstm_forward_train(mod, x).float().cpu().to(F64)       # [B, T, H]
        last = fused.lstm_last_hidden(mod, x).float().cpu().to(F64)      # [B, H]
    torch.cuda.synchronize()
    err_y = (y.transpose(0, 1) - exact).abs().max().item()
    err_last = (last - exact[-1]).abs().max().item()
    print(f"floor {floor:.3e}: lstm_forward_train {err_y:.3e} = {err_y / floor:.2f} x floor, "
          f"lstm_last_hidden {err_last:.3e} = {err_last / floor:.2f} x floor")
    assert err_y <= 3 * floor
    assert err_last <= 3 * floor


@pytest.mark.gpu
@pytest.mark.parametrize("wave", ["1", "0"])
def test_1024_steps_within_three_floors_of_exact(gpu_build, monkeypatch, wave):
    """G6: every step of a 2-layer, T = 1024 run (B = 20: a full and a partial
    row block) against the real-number reference."""
    monkeypatch.setenv("VGPU_LSTM_WAVE", wave)
    from vgpu.ops import lstm as fused
    _check_long(fused, *LONG[0])


@pytest.mark.gpu
def test_one_layer_within_three_floors_of_exact(gpu_build):
    """G6, one layer: T = 33, B = 37."""
    from vgpu.ops import lstm as fused
    _check_long(fused, *LONG[1])


@pytest.mark.gpu
@pytest.mark.parametrize("wave", ["1", "0"])
@pytest.mark.parametrize("b,t", [(16, 1), (129, 9), (17, 33), (10, 1024)])
def test_training_gradients_dense_loss(gpu_build, monkeypatch, wave, b, t):
    """G7: loss sum_t y_t . head_t, so every step's dy counts; fp64 torch.nn.LSTM
    autograd on the CPU is the reference."""
    monkeypatch.setenv("VGPU_LSTM_WAVE", wave)
    from vgpu.ops import lstm as fused
    case = _grad_case(b, t)
    mod = _gpu_lstm(case["params"], 64, 2)
    xb = case["x"].cuda().requires_grad_(True)
    (fused.lstm_forward_train(mod, xb).float() * case["head"].cuda()).sum().backward()
    torch.cuda.synchronize()
    got = {n: p.grad for n, p in mod.named_parameters()}
    got["x"] = xb.grad
    errs = {}
    for name, want in case["grads"].items():
        g = got[name].float().cpu().to(F64)
        assert bool(torch.isfinite(g).all()), name
        errs[name] = (g - want).abs().max().item() / (want.abs().max().item() + 1e-6)
    print("max-norm relative gradient error vs fp64:", {k: round(v, 4) for k, v in errs.items()})
    assert max(errs.values()) < 0.05, errs
