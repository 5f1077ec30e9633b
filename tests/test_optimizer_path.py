"""The only path by which a training step changes the model, held to float64 element by element: the flat fp32 arena
(`bioreason_amd/arena.py`) and the small kernels of k_misc.hip behind it —
    bra_sumsq -> bra_adamw (global-norm clip fused in) -> bra_pack_params,   bra_cast_grad,   bra_vec_sum,   bra_colsum.

Every reference is plain PyTorch in float64 on the CPU, computed from the very fp32 / bf16 values the kernel reads.

Bounds (none of them comes from what the kernels return):
  * sums (`sumsq`, `vec_sum`, `colsum`): the worst-case bound of an fp32 summation of k terms in any order,
    k * 2^-24 * sum|terms|; the inputs are the same fp32 values, so nothing else enters.
  * AdamW: `torch.optim.AdamW` + `clip_grad_norm_` in fp32 on the same masked, scaled gradients is the yardstick.  The kernel's
    distance to the float64 restatement may be at most 2 x the distance of that fp32 run to it (the factor covers a different
    but equally valid fp32 operation order); the moments to 1e-4 of their float64 maxima (`1 - 0.999f` alone is 1.3e-5 off).
  * casts, packs, masked-out state: bit for bit.
The sizes cross every cap of the launch code: `ew_grid` stops at 2048 blocks (524 288 elements; 32 blocks = 8192 elements in the
emulator) and `bra_sumsq` at 1024 blocks (262 144 elements); `colsum_kernel` starts a second row block at row 256.

What the hip legs found when they first ran (fixed in k_misc.hip with them): under -ffast-math the device compiler rewrote the moving
averages as g + b (m - g), which left v 4e-5 .. 6e-5 off (emulator: 1.3e-5) and the parameters up to 15 x the fp32 yardstick's error
(tiny_b step 2: 4.96e-07 against 3.29e-08; `step_1000` 4.9 x, `wd_0` 3.6 x); and the fp32 `1 - powf(b2, step)` put the emulator at
1.95 x on the same step.  With the averages kept in the written order and the bias corrections taken in double, both backends sit
at 0.90 .. 1.61 x."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_model_parity import GOLD, build, to_dev   # noqa: E402

from bioreason_amd import ops                        # noqa: E402
from bioreason_amd.arena import TrainableArena, _PackDesc   # noqa: E402

BF16 = torch.bfloat16
U = 2.0 ** -24                                        # unit round-off of fp32
B1, B2, EPS = 0.9, 0.999, 1e-8


def bits(t):
    """the raw bits of a tensor, on the CPU (NaN-proof, and -0.0 != +0.0)"""
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def byte_mask(n, gen, zeros=0.2):
    return (torch.rand(n, generator=gen) >= zeros).to(torch.uint8)


# values whose fp32 -> bf16 rounding is easy to get wrong: round-to-nearest-even ties (down to 1.0, up to 1 + 2^-6), signed zeros,
# an fp32 subnormal, and the largest magnitudes (3.4e38 rounds to inf)
SPECIALS = [1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 0.0, -0.0, 1e-40, 3.4e38, -3.4e38, -(1.0 + 2.0 ** -8)]


# =============================================================================== 1. bra_sumsq
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1024, 8192 + 77, 262144 + 77, 524288 + 333])
def test_sumsq(backend, n):
    gen = torch.Generator().manual_seed(n)
    g = torch.randn(n, generator=gen) * 1e3
    mask = byte_mask(n, gen)
    gd = g.to(backend)
    for name, mk in (("no mask", None), ("20% zeros", mask), ("all zeros", torch.zeros(n, dtype=torch.uint8))):
        keep = torch.ones(n, dtype=torch.bool) if mk is None else mk.bool()
        ref = float((g.double()[keep] ** 2).sum())
        md = None if mk is None else mk.to(backend)
        out = torch.full((1,), -12345.0, device=backend)            # a sentinel: the call overwrites, it does not accumulate
        ops.sumsq(gd, out, mask=md)
        got = float(out.double().cpu())
        err = abs(got - ref)
        print(f"sumsq n={n} {name}: got {got!r} ref {ref!r} abs err {err:.3e} (bound {n * U * ref:.3e})")
        if name == "all zeros":
            assert got == 0.0, got
        else:
            assert err <= n * U * ref, (name, got, ref, err, n * U * ref)
        out2 = torch.full((1,), 777.0, device=backend)
        ops.sumsq(gd, out2, mask=md, ws=torch.full((1024,), 3.0, device=backend))   # a dirty workspace must not matter either
        assert same_bits(out, out2), (name, float(out), float(out2))             # fixed order: the same bits every time
    # every element is visited: one non-zero anywhere gives its square exactly (the summation bound above is too loose at
    # large n to notice a dropped tail)
    for pos in sorted({0, n // 2, n - 1}):
        hot = torch.zeros(n)
        hot[pos] = 3.0
        out = torch.full((1,), -1.0, device=backend)
        ops.sumsq(hot.to(backend), out)
        assert float(out) == 9.0, (pos, float(out))


# =============================================================================== 2. bra_adamw
def f64_adamw_step(p, g, m, v, keep, step, lr, wd, max_norm, grad_scale):
    """`torch.optim.AdamW.step()` after `clip_grad_norm_(max_norm)`, restated in float64 (torch/optim/adamw.py `_single_tensor_adamw`,
    torch/nn/utils/clip_grad.py); elements outside `keep` are structural zeros: not in the norm, not updated"""
    g = g * grad_scale
    if max_norm > 0:
        nrm = math.sqrt(float((g[keep] ** 2).sum()))
        g = g * min(1.0, max_norm / (nrm + 1e-6))
    p2 = p * (1.0 - lr * wd)
    m2 = B1 * m + (1.0 - B1) * g
    v2 = B2 * v + (1.0 - B2) * g * g
    denom = v2.sqrt() / math.sqrt(1.0 - B2 ** step) + EPS
    p2 = p2 - (lr / (1.0 - B1 ** step)) * m2 / denom
    return torch.where(keep, p2, p), torch.where(keep, m2, m), torch.where(keep, v2, v)


def torch_fp32_step(p, g, m, v, step, lr, wd, max_norm):
    """the installed fp32 `torch.optim.AdamW` (+ `clip_grad_norm_`) for one step from explicit state; g is already masked and scaled"""
    q = torch.nn.Parameter(p.clone())
    q.grad = g.clone()
    if max_norm > 0:
        torch.nn.utils.clip_grad_norm_([q], max_norm)
    opt = torch.optim.AdamW([q], lr=lr, betas=(B1, B2), eps=EPS, weight_decay=wd, foreach=False)
    opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    opt.step()
    assert float(opt.state[q]["step"]) == step
    return q.detach().clone(), opt.state[q]["exp_avg"].clone(), opt.state[q]["exp_avg_sq"].clone()


def kernel_step(p, g, m, v, mask, step, lr, wd, max_norm, grad_scale, use_sumsq=True):
    ss = None
    if use_sumsq:
        ss = torch.zeros(1, device=p.device)
        ops.sumsq(g, ss, mask=mask)
    ops.adamw(p, g, m, v, lr, B1, B2, EPS, wd, step, sumsq_t=ss, max_norm=max_norm, grad_scale=grad_scale, mask=mask)


def assert_within_twice_fp32(what, got, tor, ref):
    """max|kernel - f64| <= 2 x max|torch_fp32 - f64| (both float64 tensors of the same elements)"""
    e_k = float((got - ref).abs().max())
    e_t = float((tor - ref).abs().max())
    print(f"{what}: max|kernel - f64| = {e_k:.4e}, max|torch_fp32 - f64| = {e_t:.4e}, ratio {e_k / e_t if e_t else float('nan'):.3f}")
    assert e_k <= 2.0 * e_t, f"{what}: max|kernel - f64| = {e_k:.4e} > 2 x max|torch_fp32 - f64| = {e_t:.4e}"


def grads_big(n, gen):
    return torch.randn(n, generator=gen) * 3


def grads_eps(n, gen):
    return torch.randn(n, generator=gen) * 1e-8          # sqrt(v) ~ eps: where eps sits in the denominator shows


def grads_logspace(n, gen):
    return torch.randn(n, generator=gen) * torch.logspace(-10, 1, n)


ADAMW_CASES = {
    # name: (n, steps, gradients, weight decay, first step, mask)
    "scale_3": (3 * 8192 + 77, 7, grads_big, 0.01, 1, True),
    "scale_1e-8": (3 * 8192 + 77, 7, grads_eps, 0.01, 1, True),
    "scale_logspace": (3 * 8192 + 77, 7, grads_logspace, 0.01, 1, True),
    "past_grid_cap": (524288 + 333, 2, grads_big, 0.01, 1, True),
    "n_1": (1, 7, grads_big, 0.01, 1, False),
    "n_257": (257, 7, grads_big, 0.01, 1, True),
    "wd_0": (3 * 8192 + 77, 7, grads_big, 0.0, 1, True),
    "step_1000": (3 * 8192 + 77, 2, grads_big, 0.01, 1000, True),
}


@pytest.mark.parametrize("case", list(ADAMW_CASES))
def test_adamw_against_float64(backend, case):
    n, steps, make, wd, first, masked = ADAMW_CASES[case]
    lr, max_norm, grad_scale = 1e-2, 1.0, 0.5
    gen = torch.Generator().manual_seed(11)
    p0 = torch.randn(n, generator=gen)
    mask = byte_mask(n, gen) if masked else torch.ones(n, dtype=torch.uint8)
    keep = mask.bool()
    assert keep.any() and (not masked or not keep.all())
    p, m, v = p0.clone().to(backend), torch.zeros(n, device=backend), torch.zeros(n, device=backend)
    md = mask.to(backend)
    rp, rm, rv = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    tp, tm, tv = p0[keep].clone(), torch.zeros(int(keep.sum())), torch.zeros(int(keep.sum()))
    for step in range(first, first + steps):
        g = make(n, gen)
        kernel_step(p, g.to(backend), m, v, md, step, lr, wd, max_norm, grad_scale)
        rp, rm, rv = f64_adamw_step(rp, g.double(), rm, rv, keep, step, lr, wd, max_norm, grad_scale)
        tp, tm, tv = torch_fp32_step(tp, (g * grad_scale)[keep], tm, tv, step, lr, wd, max_norm)    # 0.5 g is exact
    assert_within_twice_fp32(f"adamw {case} p", p.double().cpu()[keep], tp.double(), rp[keep])
    for nm, got, ref in (("m", m, rm), ("v", v, rv)):
        e, top = float((got.double().cpu() - ref)[keep].abs().max()), float(ref[keep].abs().max())
        print(f"adamw {case} {nm}: max err {e:.3e} = {e / top:.3e} of max {top:.3e}")
        assert e <= 1e-4 * top, (nm, e, top)
    # structural zeros: parameter and moments exactly as they were
    assert same_bits(p.cpu()[~keep], p0[~keep])
    assert not m.cpu()[~keep].any() and not v.cpu()[~keep].any()


def _state(n, dev, seed=5):
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen)
    m = torch.randn(n, generator=gen) * 0.1
    v = torch.rand(n, generator=gen) * 0.01
    g = torch.randn(n, generator=gen)
    mask = byte_mask(n, gen)
    return [t.to(dev) for t in (p, m, v, g, mask)]


def test_adamw_inactive_clip_is_no_clip(backend):
    """||grad_scale g|| < max_norm: the clip factor must be exactly 1 — the same bits as a call without the norm, or with max_norm = 0"""
    n = 8192 + 77
    p, m, v, g, mask = _state(n, backend)
    g = g * 1e-3                                           # ||g|| ~ 0.09
    ss = torch.zeros(1, device=backend)
    ops.sumsq(g, ss, mask=mask)
    assert 0 < math.sqrt(float(ss)) * 0.5 < 1.0
    out = []
    for kw in (dict(sumsq_t=ss, max_norm=1.0), dict(sumsq_t=None, max_norm=1.0), dict(sumsq_t=ss, max_norm=0.0)):
        q, a, b = p.clone(), m.clone(), v.clone()
        ops.adamw(q, g, a, b, 1e-2, B1, B2, EPS, 0.01, 3, grad_scale=0.5, mask=mask, **kw)
        out.append((q, a, b))
    assert not same_bits(out[0][0], p)                     # (it did step)
    for other in out[1:]:
        for x, y in zip(out[0], other):
            assert same_bits(x, y)


@pytest.mark.parametrize("clip", [True, False])
def test_adamw_grad_scale_is_a_scaled_gradient(backend, clip):
    """grad_scale = s on g  ==  grad_scale = 1 on s g, bit for bit when s is a power of two (every product by s is exact); the scale
    enters the clip norm too"""
    n, s = 8192 + 77, 0.125
    p, m, v, g, mask = _state(n, backend)
    g = g * (3.0 if clip else 1e-3)
    res = []
    for gg, scale in ((g, s), (g * s, 1.0)):
        q, a, b = p.clone(), m.clone(), v.clone()
        kernel_step(q, gg, a, b, mask, 4, 1e-2, 0.01, 1.0, scale)
        res.append((q, a, b))
    for x, y in zip(*res):
        assert same_bits(x, y)
    # and it is not the unscaled step
    q, a, b = p.clone(), m.clone(), v.clone()
    kernel_step(q, g, a, b, mask, 4, 1e-2, 0.01, 1.0, 1.0)
    assert not same_bits(a, res[0][1])


def test_adamw_zero_gradients_without_decay_change_nothing(backend):
    n = 8192 + 77
    p = _state(n, backend)[0]
    p0 = p.clone()
    m, v, g = torch.zeros(n, device=backend), torch.zeros(n, device=backend), torch.zeros(n, device=backend)
    for step in (1, 2):
        kernel_step(p, g, m, v, None, step, 1e-2, 0.0, 1.0, 0.5)
    assert same_bits(p, p0)
    assert same_bits(m, torch.zeros(n)) and same_bits(v, torch.zeros(n))


def test_adamw_never_touches_masked_out_elements(backend):
    """weight decay on, large gradients in the masked-out slots (as the weight-gradient kernels leave them in the off-diagonal blocks
    of a fused LoRA B): parameter and both moments keep their bits there, and those gradients stay out of the clip norm"""
    n = 3 * 8192 + 77
    p, _, _, g, mask = _state(n, backend)
    on = mask.bool()
    keep = on.cpu()
    g = torch.where(on, g, torch.full_like(g, 1e6))
    # fresh moments where the step acts, recognisable values where it must not
    m = torch.where(on, torch.zeros_like(p), torch.full_like(p, 7.0))
    v = torch.where(on, torch.zeros_like(p), torch.full_like(p, 9.0))
    p0, m0, v0 = p.clone(), m.clone(), v.clone()
    kernel_step(p, g, m, v, mask, 1, 1e-2, 0.1, 1.0, 1.0)
    for now, was in ((p, p0), (m, m0), (v, v0)):
        assert same_bits(now.cpu()[~keep], was.cpu()[~keep])
        assert not torch.equal(now.cpu()[keep], was.cpu()[keep])
    # nothing of the 1e6 entered the norm: the masked-in elements moved as AdamW + clip over them alone moves them, in the full
    # layout and compacted into a tensor of their own without a mask
    q, a, b = p0[on].clone(), m0[on].clone(), v0[on].clone()
    kernel_step(q, g[on].clone(), a, b, None, 1, 1e-2, 0.1, 1.0, 1.0)
    rp, _, _ = f64_adamw_step(p0.double().cpu(), g.double().cpu(), m0.double().cpu(), v0.double().cpu(), keep, 1, 1e-2, 0.1, 1.0, 1.0)
    tp, _, _ = torch_fp32_step(p0.cpu()[keep], g.cpu()[keep], m0.cpu()[keep], v0.cpu()[keep], 1, 1e-2, 0.1, 1.0)
    assert_within_twice_fp32("adamw masked p", p.double().cpu()[keep], tp.double(), rp[keep])
    assert_within_twice_fp32("adamw compacted p", q.double().cpu(), tp.double(), rp[keep])


# =============================================================================== 3. bra_pack_params
PACK_SHAPES = [(1, 1), (3, 257), (64, 2048), (130, 96), (1, 300)]


def _desc_table(entries, dev):
    arr = (_PackDesc * len(entries))()
    for i, (s, d, t) in enumerate(entries):
        arr[i] = _PackDesc(s.data_ptr(), s.stride(0), d.data_ptr(), d.stride(0), s.shape[0], s.shape[1], int(t), 0)
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).clone().to(dev)


@pytest.mark.parametrize("first_transposed", [False, True])
def test_pack_params_table(backend, first_transposed):
    """descriptors of very different sizes share one grid sized by the largest; plain and transposed alternate; sources are cut from
    wider fp32 buffers (src_ld > cols) and destinations are windows of one larger bf16 buffer (dst_ld > cols, or > rows transposed)"""
    gen = torch.Generator().manual_seed(3)
    srcs, wins, off = [], [], 5
    for i, (r, c) in enumerate(PACK_SHAPES):
        t = bool((i + int(first_transposed)) % 2)
        wide = torch.randn(r, c + 3 + i, generator=gen)
        s = wide[:, 2:2 + c]
        for k, val in enumerate(SPECIALS[:r * c]):
            s[(k * 7) % r, (k * 5 + k // c) % c] = val          # scattered over rows and columns
        R, C = (c, r) if t else (r, c)
        ld = C + 1 + 2 * i
        wins.append((off, R, C, ld, t))
        off += R * ld + 11
        srcs.append(wide)
    total = off
    sentinel = ((torch.arange(total, dtype=torch.int32) * 37 + 11) % 30011).to(torch.int16)      # finite, never zero-extended junk
    buf = sentinel.clone().to(backend).view(BF16)
    want = sentinel.clone().view(BF16)
    entries, keep_alive = [], []
    for wide, (o, R, C, ld, t), (r, c) in zip(srcs, wins, PACK_SHAPES):
        assert o + R * ld <= total
        wd_ = wide.to(backend)
        keep_alive.append(wd_)
        s_dev = wd_[:, 2:2 + c]
        d_dev = buf[o:o + R * ld].view(R, ld)[:, :C]
        assert s_dev.stride(0) > c and d_dev.stride(0) > C
        entries.append((s_dev, d_dev, t))
        img = wide[:, 2:2 + c].to(BF16)
        want[o:o + R * ld].view(R, ld)[:, :C] = img.T if t else img
    table = _desc_table(entries, backend)
    mx = max(r * c for r, c in PACK_SHAPES)
    ops.pack_params(table, 0, mx)                              # ndesc = 0: a no-op
    assert torch.equal(bits(buf), sentinel)
    ops.pack_params(table, len(entries), mx)
    for (s_dev, d_dev, t), (r, c) in zip(entries, PACK_SHAPES):
        img = s_dev.cpu().to(BF16)
        assert torch.equal(d_dev.cpu(), img.T if t else img), ((r, c), t)
        assert same_bits(d_dev.cpu().contiguous(), (img.T if t else img).contiguous()), ((r, c), t)      # -0.0 stays -0.0
    bad = (bits(buf) != bits(want)).nonzero().flatten()
    assert bad.numel() == 0, f"{bad.numel()} elements differ, first at {bad[:8].tolist()} (windows: {wins})"
    inf = want.float().isinf().sum().item()
    assert inf >= 2 * 4                                        # 3.4e38 did round to inf in the images that hold it


# =============================================================================== 4. bra_cast_grad
@pytest.mark.parametrize("n", [1, 255, 256, 257, 70001])
def test_cast_grad(backend, n):
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=gen) * torch.logspace(-3, 3, n)
    extra = SPECIALS + [float("inf"), float("-inf"), float("nan")]
    k = min(n, len(extra))
    x[:k] = torch.tensor(extra[:k]) if n > 1 else torch.tensor([1.0 + 2.0 ** -8])
    # fp32 -> bf16
    dst = torch.full((n + 1,), 7.0, dtype=BF16, device=backend)
    ops.cast_grad(x.to(backend), dst[:n])
    want = x.to(BF16)
    got = dst.cpu()
    nan = want.isnan()
    assert torch.equal(got[:n].isnan(), nan)
    assert torch.equal(bits(got[:n])[~nan], bits(want)[~nan]), (bits(got[:n]) != bits(want)).nonzero().flatten()[:8].tolist()
    assert float(got[n]) == 7.0                                # the element past n stays
    # bf16 -> fp32, every kind of bit pattern
    hb = torch.randint(-32768, 32768, (n,), generator=gen, dtype=torch.int32).to(torch.int16)
    hb[:k] = bits(want)[:k]
    h = hb.view(BF16)
    dst32 = torch.full((n + 1,), 7.0, device=backend)
    ops.cast_grad(h.to(backend), dst32[:n])
    got32, want32 = dst32.cpu(), h.float()
    nan = want32.isnan()
    assert torch.equal(got32[:n].isnan(), nan)
    assert torch.equal(bits(got32[:n])[~nan], bits(want32)[~nan])
    assert float(got32[n]) == 7.0
    # bf16 -> fp32 -> bf16 is the identity
    back = torch.full((n + 1,), 7.0, dtype=BF16, device=backend)
    ops.cast_grad(dst32[:n], back[:n])
    b = back.cpu()
    assert torch.equal(b[:n].isnan(), nan)
    assert torch.equal(bits(b[:n])[~nan], hb[~nan])
    assert float(b[n]) == 7.0


# =============================================================================== 5. bra_vec_sum, bra_colsum
@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000])
@pytest.mark.parametrize("mean", [False, True])
def test_vec_sum(backend, n, mean):
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=gen)
    scale = float(np.float32(-1.0 / n)) if mean else 1.0       # the fp32 the kernel receives
    got = float(ops.vec_sum(x.to(backend), scale).double().cpu())
    ref = float(x.double().sum()) * scale
    bound = n * U * float(x.double().abs().sum()) * abs(scale) + float(np.spacing(np.float32(abs(ref))))
    print(f"vec_sum n={n} scale={scale}: got {got!r} ref {ref!r} err {abs(got - ref):.3e} bound {bound:.3e}")
    assert abs(got - ref) <= bound, (got, ref, abs(got - ref), bound)


@pytest.mark.parametrize("rows", [1, 255, 256, 257, 700])
@pytest.mark.parametrize("cols,pitch", [(100, 104), (256, 256), (300, 300)])
def test_colsum_accumulates(backend, rows, cols, pitch):
    """rows >= 257: the second row block and the cross-block atomicAdd; cols = 300: a second column block with a ragged end"""
    gen = torch.Generator().manual_seed(rows * 1000 + cols)
    x = torch.randn(rows, pitch, generator=gen).to(BF16)
    out0 = torch.randn(cols + 1, generator=gen)
    out = out0.clone().to(backend)
    xd = x.to(backend)[:, :cols]
    assert xd.stride(0) == pitch
    ops.colsum(xd, out[:cols])
    xs = x[:, :cols].double()
    ref = xs.sum(0) + out0[:cols].double()
    bound = (rows + 1) * U * (xs.abs().sum(0) + out0[:cols].double().abs())
    err = (out.double().cpu()[:cols] - ref).abs()
    print(f"colsum {rows}x{cols}: max err / bound = {float((err / bound).max()):.3e}")
    assert bool((err <= bound).all()), (int((err > bound).sum()), float((err / bound).max()))
    assert float(out[cols]) == float(out0[cols])              # nothing past the last column


# =============================================================================== 6. TrainableArena as a whole
ARENA_BLOCKS = [("a", 5, 13), ("b", 1, 70), ("bcat", 33, 64), ("d", 64, 7)]


class _Owner:
    """what a module that owns arena blocks does: set its mask and (re)register its bf16 images at every (re)bind"""

    def __init__(self, arena):
        self.arena, self.images = arena, {}
        arena.on_rebind(self.bind)

    def bind(self):
        a = self.arena
        for nm in a._shapes:
            if nm != "bcat":
                a.mask_view(nm).fill_(1)
        bm = a.mask_view("bcat")                    # two diagonal blocks of a fused B; the off-diagonal blocks belong to no adapter
        bm.zero_()
        bm[:20, :32] = 1
        bm[20:, 32:] = 1
        dev = a.device
        self.images = {"a": torch.zeros(5, 13, dtype=BF16, device=dev),
                       "bcatT": torch.zeros(64, 40, dtype=BF16, device=dev)[:, :33],
                       "d": torch.zeros(64, 16, dtype=BF16, device=dev)[:, :7],
                       "bT": torch.zeros(70, 1, dtype=BF16, device=dev)}
        a.register_pack(a.param("a"), self.images["a"], False)
        a.register_pack(a.param("bcat"), self.images["bcatT"], True)
        a.register_pack(a.param("d"), self.images["d"], False)
        a.register_pack(a.param("b"), self.images["bT"], True)


def _images_fresh(arena):
    assert arena._packs
    for src, dst, t in arena._packs:
        img = src.cpu().to(BF16)
        assert torch.equal(dst.cpu(), img.T if t else img)


def test_arena_steps_growth_and_images(backend, monkeypatch):
    lr, wd, max_norm, scale = 1e-2, 0.01, 1.0, 0.25
    gen = torch.Generator().manual_seed(9)
    A = TrainableArena(backend)
    for nm, r, c in ARENA_BLOCKS:
        A.add(nm, r, c)
    own = _Owner(A)
    A.commit()
    N = A.numel
    assert N == 128 + 128 + 2112 + 448 and len(A._packs) == 4
    keep = A.mask.bool().cpu()
    assert int(keep.sum()) == 65 + 70 + (20 * 32 + 13 * 32) + 448
    assert not keep[65:128].any() and not keep[128 + 70:256].any()       # the padding gaps are real and masked out
    p0 = torch.randn(N, generator=gen)
    A.params.copy_(p0)                                                 # noise in the masked-out slots and the padding too
    A.exp_avg = torch.where(A.mask.bool(), torch.zeros_like(A.params), torch.full_like(A.params, 7.0))
    A.exp_avg_sq = torch.where(A.mask.bool(), torch.zeros_like(A.params), torch.full_like(A.params, 9.0))
    m0, v0 = A.exp_avg.cpu().clone(), A.exp_avg_sq.cpu().clone()
    rp, rm, rv = p0.double(), torch.zeros(N, dtype=torch.float64), torch.zeros(N, dtype=torch.float64)
    tp, tm, tv = p0[keep].clone(), torch.zeros(int(keep.sum())), torch.zeros(int(keep.sum()))

    def step_and_check(step, keep, rp, rm, rv, tp, tm, tv, p_init, m_init, v_init):
        n = A.numel
        g = torch.randn(n, generator=gen) * 2                          # ALL of the gradient buffer, padding and masked-out slots too
        A.grads.copy_(g)
        ref_norm = math.sqrt(float((g.double()[keep] ** 2).sum()))
        got_norm = float(A.grad_norm().double().cpu())
        # sumsq within n 2^-24 (section 1), so the root within half of that, plus the root's own rounding
        assert abs(got_norm - ref_norm) <= (n / 2 + 1) * U * ref_norm, (got_norm, ref_norm)
        A.adamw_step(lr, (B1, B2), EPS, wd, max_grad_norm=max_norm, grad_scale=scale)
        assert A.step_count == step
        rp, rm, rv = f64_adamw_step(rp, g.double(), rm, rv, keep, step, lr, wd, max_norm, scale)
        tp, tm, tv = torch_fp32_step(tp, (g * scale)[keep], tm, tv, step, lr, wd, max_norm)
        assert_within_twice_fp32(f"arena step {step} p", A.params.double().cpu()[keep], tp.double(), rp[keep])
        for now, was in ((A.params, p_init), (A.exp_avg, m_init), (A.exp_avg_sq, v_init)):
            assert same_bits(now.cpu()[~keep], was[~keep])
        _images_fresh(A)
        return rp, rm, rv, tp, tm, tv

    for step in range(1, 6):
        rp, rm, rv, tp, tm, tv = step_and_check(step, keep, rp, rm, rv, tp, tm, tv, p0, m0, v0)

    # ---- growth: a fifth block; the old state survives, the new block starts from zero moments at the arena's step count
    before = [t.cpu().clone() for t in (A.params, A.exp_avg, A.exp_avg_sq)]
    A.add("e", 7, 11)
    A.commit()
    assert A.numel == N + 128 and A.step_count == 5 and len(A._packs) == 4
    for now, was in zip((A.params, A.exp_avg, A.exp_avg_sq), before):
        assert same_bits(now.cpu()[:N], was)
    assert not A.exp_avg[N:].any() and not A.exp_avg_sq[N:].any() and not A.params[N:].any()
    e0 = torch.randn(7, 11, generator=gen)
    A.param("e").copy_(e0)
    keep2 = A.mask.bool().cpu()
    assert torch.equal(keep2[:N], keep) and int(keep2[N:].sum()) == 77
    # the references go on: step 6 for the old elements, zero moments for the new ones
    z128, z77 = torch.zeros(128, dtype=torch.float64), torch.zeros(77)
    rp, rm, rv = torch.cat([rp, A.params[N:].double().cpu()]), torch.cat([rm, z128]), torch.cat([rv, z128])
    tp, tm, tv = torch.cat([tp, e0.flatten()]), torch.cat([tm, z77]), torch.cat([tv, z77])
    p_init = A.params.cpu().clone()
    m_init, v_init = A.exp_avg.cpu().clone(), A.exp_avg_sq.cpu().clone()
    A.pack_if_stale()
    step_and_check(6, keep2, rp, rm, rv, tp, tm, tv, p_init, m_init, v_init)

    # ---- pack_if_stale: one launch after an in-place torch write to the master, none when nothing changed
    calls = []
    real = ops.pack_params
    monkeypatch.setattr(ops, "pack_params", lambda *a, **k: (calls.append(a), real(*a, **k))[1])
    A.pack_if_stale()
    assert calls == []
    A.param("bcat").mul_(1.5)
    A.param("a")[2, 3] = 1.0 + 3 * 2.0 ** -8
    with pytest.raises(AssertionError):
        _images_fresh(A)                                               # stale now
    A.pack_if_stale()
    assert len(calls) == 1
    _images_fresh(A)
    A.pack_if_stale()
    assert len(calls) == 1
    assert float(own.images["a"][2, 3]) == 1.0 + 2.0 ** -6              # the tie rounded to even


# =============================================================================== 7. the real model: three SFT steps on tiny_b
def test_three_sft_steps_on_tiny_b(backend):
    """weights after a step: the arena's clip norm is `clip_grad_norm_` over the NAMED parameters, the named parameters move as AdamW
    moves them, the structural zeros of the fused LoRA factors stay zero although their gradient slots are filled, and no bf16 image
    is left stale"""
    from bioreason_amd.trainer import SFTStepRunner
    fix = torch.load(os.path.join(GOLD, "tiny_b.pt"), weights_only=False)
    m = build(fix, backend, True)
    m.train()
    A = m.arena
    lr, wd = 1e-2, 0.01
    runner = SFTStepRunner(m, learning_rate=lr, weight_decay=wd)
    named = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
    total = sum(p.numel() for _, p in named)
    assert int(A.mask.sum()) == total, (int(A.mask.sum()), total)      # the mask marks exactly the named trainable elements
    seen = []
    orig = A.adamw_step

    def spy(lr_, *a, **kw):
        assert all(p.grad is not None for _, p in named)
        seen.append({"lr": lr_, "args": a, "kw": kw,
                     "p": torch.cat([p.detach().double().cpu().flatten() for _, p in named]),
                     "g": torch.cat([p.grad.detach().double().cpu().flatten() for _, p in named]),
                     "arena_norm": float(A.grad_norm().double().cpu()),
                     "masked_out_nonzero": int((A.grads[A.mask == 0] != 0).sum())})
        return orig(lr_, *a, **kw)
    A.adamw_step = spy
    batch = to_dev(fix["batch"], backend)
    rm, rv = torch.zeros(total, dtype=torch.float64), torch.zeros(total, dtype=torch.float64)
    tm, tv = torch.zeros(total), torch.zeros(total)
    everything = torch.ones(total, dtype=torch.bool)
    losses = []
    try:
        for step in range(1, 4):
            res = runner.step(batch)
            assert res.get("stepped") and len(seen) == step
            losses.append(float(res["loss_t"]))
            rec = seen[-1]
            betas, eps, wd_ = rec["args"][:3]
            assert (tuple(betas), eps, wd_, rec["lr"]) == ((B1, B2), EPS, wd, lr)
            max_norm, scale = rec["kw"]["max_grad_norm"], rec["kw"]["grad_scale"]
            assert max_norm == 1.0
            # clip norm
            named_norm = math.sqrt(float((rec["g"] ** 2).sum()))
            print(f"step {step}: loss {losses[-1]:.4f} arena norm {rec['arena_norm']!r} named float64 norm {named_norm!r} "
                  f"masked-out non-zero gradients {rec['masked_out_nonzero']}")
            assert abs(rec["arena_norm"] - named_norm) <= 1e-6 * named_norm, (rec["arena_norm"], named_norm)
            assert rec["masked_out_nonzero"] > 0                       # or this test no longer tests what it claims
            # named parameters against AdamW
            rp, rm, rv = f64_adamw_step(rec["p"], rec["g"], rm, rv, everything, step, lr, wd, max_norm, scale)
            tp, tm, tv = torch_fp32_step(rec["p"].float(), (rec["g"] * scale).float(), tm, tv, step, lr, wd, max_norm)
            now = torch.cat([p.detach().double().cpu().flatten() for _, p in named])
            assert_within_twice_fp32(f"tiny_b step {step} named parameters", now, tp.double(), rp)
            # structural zeros
            out = (A.mask == 0)
            for t in (A.params, A.exp_avg, A.exp_avg_sq):
                assert not t[out].any()
            _images_fresh(A)
    finally:
        A.adamw_step = orig
    assert len(A._packs) >= 10
    assert losses[-1] < losses[0], losses
    # the pack after an optimiser step equals the pack after a load
    m2 = build(fix, backend, True)
    m2.arena.params.copy_(A.params)
    m2.arena.pack_if_stale()
    _images_fresh(m2.arena)
    m.eval()
    m2.eval()
    with torch.no_grad():
        l1, l2 = m(**batch).loss, m2(**batch).loss
    assert same_bits(l1.float(), l2.float()), (float(l1), float(l2))
