"""bra_grpo_loss_is (ops.grpo_loss_is, grpo.grpo_loss(rollout_logp=...)) — the GRPO loss with truncated importance sampling against
the rollout's own log-probs — against float64 autograd, element by element.

Per token, with q = old_logp (logp where there is none) and w = min(exp(q - rollout_logp), is_cap) a constant for the gradient:
    loss_t = w (-min(l1, l2)) + beta kl,        dlogp = (w g_pg + beta (1 - e)) mask / (ms B)
out6 = {loss, mean_kl, clip_ratio, is_mean, is_capped, rollout_kl}.

Criterion: the element-wise dlogp bound and the out bounds of tests/test_loss_path_rowwise.py::test_grpo_loss_elementwise, restated
here for the formula above — the policy term carries w's roundings too (its exponential 2 u, the exponent q - rollout_logp and its
product with log2 e (1 + 1.5) u |dw| -> 3 u |dw|, the product w g under -ffast-math 3 u): (7 + 3 |d|) becomes (12 + 3 |d| + 3 |dw|).
The allowed ratio for dlogp is twice the worst ratio of an fp32 torch twin of the kernel's statements, measured in this file over
every case; the sums (loss, kl, is_mean, rollout_kl) are held to worst-case bounds, ratio <= 1 without a margin.
Where rollout_logp equals q bit for bit, out6[0..3) and dlogp are ops.grpo_loss's bits, on every case.
"""
import functools
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from bioreason_amd import grpo, ops                                    # noqa: E402
from bioreason_amd._lib import BRA_ERR_ARG, KernelError, current_stream, get_lib      # noqa: E402
from oracle import grpo_math                                           # noqa: E402

F32, F64 = torch.float32, torch.float64
U32 = 2.0 ** -24
EPS_LO, EPS_HI = 0.2, 0.3
SHAPES = [(1, 1), (4, 255), (4, 257), (8, 700)]
CAPS = [1.0, 2.0, 1e30]
CASES = [(B, C, use_old, beta, cap) for (B, C) in SHAPES for use_old in (False, True) for beta in (0.0, 0.04) for cap in CAPS]


@functools.lru_cache(maxsize=None)
def _inputs(B, C, use_old, cap):
    """fp32 inputs on the CPU: logp / old / ref / advantages / masks as the grpo-loss test of tests/test_loss_path_rowwise.py places them
    (clamp edges 16 fp32 ulp inside and outside, far inside / outside, the tie), and rollout_logp = q - log w with log w from a pattern:
    exactly 0 (w = 1: AT the cap for is_cap = 1, the only cap an fp32 exponential reaches exactly and portably), under the cap, over
    it, 16 fp32 ulp on either side of it (is_cap = 2), far over it (is_cap = 1e30: nothing is capped)."""
    g = torch.Generator().manual_seed(100 * B + C)
    lp = -torch.rand(B, C, generator=g) * 3
    ref = lp + 0.2 * torch.randn(B, C, generator=g)
    adv = torch.tensor([0.0, 1.3, -0.7, 50.0, -2.5, 0.4, -50.0, 1e-3])[:B].clone()
    if B == 1:
        adv = torch.tensor([1.3])
    lo, hi = 1 - float(torch.tensor(EPS_LO, dtype=F32)), 1 + float(torch.tensor(EPS_HI, dtype=F32))
    d8 = 16 * 2.0 ** -23
    logr = [math.log(lo * (1 + d8)), math.log(lo * (1 - d8)), math.log(hi * (1 - d8)), math.log(hi * (1 + d8)),
            0.05, -0.1, math.log(0.5), math.log(1.9), 0.0, 0.2, -0.15, 0.0]
    old = None
    if use_old:
        pat = torch.tensor(logr, dtype=F64)[(torch.arange(B * C) * 5 % len(logr)).view(B, C)]
        old = (lp.to(F64) - pat).to(F32)
        old[pat == 0] = lp[pat == 0]
    mask = torch.zeros(B, C, dtype=torch.int32)
    for b in range(B):
        n = C if b == B - 1 else 1 + (b * (C - 1)) // max(B - 1, 1)
        mask[b, :n] = 1
    q = old if old is not None else lp
    edge = math.log(cap) if cap < 1e20 else 3.0
    logw = [0.0, -0.3, 0.2, edge + 0.1, edge - 0.1, edge + math.log1p(d8), edge + math.log1p(-d8), 1.5, -1.0, 0.0, 0.02]
    patw = torch.tensor(logw, dtype=F64)[(torch.arange(B * C) * 7 % len(logw)).view(B, C)]
    rl = (q.to(F64) - patw).to(F32)
    rl[patw == 0] = q[patw == 0]
    return lp, old, ref, adv, mask, rl


def _edges():
    one = torch.tensor(1.0, dtype=F32)
    return float(one - torch.tensor(EPS_LO, dtype=F32)), float(one + torch.tensor(EPS_HI, dtype=F32))


def _reference(lp, old, ref, adv, mask, rl, beta, cap):
    """float64 oracle: oracle/grpo_math.grpo_loss's statements with the weight w on the policy term, autograd for dlogp"""
    lo, hi = _edges()
    B, C = lp.shape
    lpt = lp.to(F64).requires_grad_(True)
    q = (old if old is not None else lp).to(F64)
    m = mask.to(F64)
    ms = m.sum(1, keepdim=True)
    A = adv.to(F64)[:, None]
    we = torch.exp(q - rl.to(F64))
    w = torch.clamp(we, max=float(cap))
    c1 = torch.exp(lpt - q)
    c2 = torch.clamp(c1, lo, hi)
    l1, l2 = c1 * A, c2 * A
    ptl = w * -torch.min(l1, l2)
    dl = ref.to(F64) - lpt
    e = torch.exp(dl)
    kl = e - dl - 1 if beta > 0 else torch.zeros_like(e)
    tot = ptl + beta * kl
    loss = ((tot * m).sum(1) / ms[:, 0]).mean()
    loss.backward()
    # the unweighted loss of oracle/grpo_math at w = 1 is the same statement: checked once here so the oracle cannot drift from it
    l0, _, clip = grpo_math.grpo_loss(lp.to(F64), old.to(F64) if old is not None else None, ref.to(F64), adv.to(F64), m, 1 - lo, hi - 1, beta)
    with torch.no_grad():
        l_w1 = (((-torch.min(l1, l2) + beta * kl) * m).sum(1) / ms[:, 0]).mean()
        assert abs(l_w1.item() - l0.item()) <= 1e-12 * max(1.0, abs(l0.item()))
        d = (lpt - q).abs()
        dw = (q - rl.to(F64)).abs()
        c1d = c1.detach()
        inside = (c1d >= lo) & (c1d <= hi)
        unclipped = inside | ((c1d < lo) & (adv[:, None] > 0)) | ((c1d > hi) & (adv[:, None] < 0))
        Aa = A.abs()
        E = U32 * (w * Aa * c1d * unclipped * (12 + 3 * d + 3 * dw) + beta * (e * (2 + 3 * dl.abs()) + 6 * (1 - e).abs())) * m / (ms * B)
        nadd = -(-C // 256) + 6 + 4 + 3 + B
        per = (w * Aa * c1d * (13 + 3 * d + 3 * dw) + beta * (e * (8 + 3 * dl.abs()) + dl.abs() + 1)) + nadd * tot.abs()
        E_loss = U32 * ((per * m).sum(1) / ms[:, 0]).mean().item() + U32 * abs(loss.item())
        per_kl = e * (8 + 3 * dl.abs()) + dl.abs() + 1 + nadd * kl.abs()
        E_kl = U32 * ((per_kl * m).sum(1) / ms[:, 0]).mean().item()
        # is_mean: w's own roundings (5 + 3 |dw|) and the additions that carry it; rollout_kl: one subtraction per term, then the sums
        # (signed terms: the bound goes by their magnitudes)
        E_is = U32 * (((w * (5 + 3 * dw + nadd)) * m).sum(1) / ms[:, 0]).mean().item()
        E_rkl = U32 * (((dw * (2 + nadd)) * m).sum(1) / ms[:, 0]).mean().item()
        is_mean = ((w * m).sum(1) / ms[:, 0]).mean().item()
        is_capped = (((we > cap).to(F64) * m).sum() / m.sum()).item()
        rkl = (((rl.to(F64) - q) * m).sum(1) / ms[:, 0]).mean().item()
    return {"loss": loss.item(), "kl": ((kl * m).sum(1) / ms[:, 0]).mean().item(), "clip": clip.item(), "dlogp": lpt.grad, "E": E,
            "E_loss": E_loss, "E_kl": E_kl, "is_mean": is_mean, "is_capped": is_capped, "rollout_kl": rkl, "E_is": E_is, "E_rkl": E_rkl}


def _twin(lp, old, ref, adv, mask, rl, beta, cap):
    """float32 torch restatement of grpo_loss_is_kernel's dlogp"""
    one = torch.tensor(1.0, dtype=F32)
    lo, hi = one - torch.tensor(EPS_LO, dtype=F32), one + torch.tensor(EPS_HI, dtype=F32)
    B, C = lp.shape
    A = adv[:, None]
    q = old if old is not None else lp
    w = torch.minimum(torch.exp(q - rl), torch.tensor(cap, dtype=F32))
    c1 = torch.exp(lp - q)
    c2 = torch.minimum(torch.maximum(c1, lo), hi)
    l1, l2 = c1 * A, c2 * A
    g1 = -A * c1
    g2 = torch.where((c1 >= lo) & (c1 <= hi), g1, torch.zeros_like(g1))
    gg = w * torch.where(l1 < l2, g1, torch.where(l1 > l2, g2, 0.5 * (g1 + g2)))
    if beta:
        gg = gg + torch.tensor(beta, dtype=F32) * (1 - torch.exp(ref - lp))
    mk = mask.to(F32)
    return gg * mk / (mk.sum(1, keepdim=True) * B)


def _ratio(err, E):
    r = torch.where(E > 0, err / E.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return r.max().item() if r.numel() else 0.0


@functools.lru_cache(maxsize=None)
def _twin_worst():
    worst = 0.0
    for (B, C, use_old, beta, cap) in CASES:
        args = _inputs(B, C, use_old, cap)
        r = _reference(*args, beta, cap)
        worst = max(worst, _ratio((_twin(*args, beta, cap).to(F64) - r["dlogp"]).abs(), r["E"]))
    return worst


def _dev_args(dev, lp, old, ref, adv, mask, rl, beta):
    return (lp.to(dev), old.to(dev) if old is not None else None, ref.to(dev) if beta else None, adv.to(dev), mask.to(dev), rl.to(dev))


@pytest.mark.parametrize("B,C,use_old,beta,cap", CASES)
def test_grpo_loss_is_elementwise(backend, B, C, use_old, beta, cap):
    dev = backend
    lp, old, ref, adv, mask, rl = _inputs(B, C, use_old, cap)
    r = _reference(lp, old, ref, adv, mask, rl, beta, cap)
    a = _dev_args(dev, lp, old, ref, adv, mask, rl, beta)
    out6, dlogp = ops.grpo_loss_is(a[0], a[1], a[2], a[3], a[4], a[5], EPS_LO, EPS_HI, beta, cap)
    out6b, none = ops.grpo_loss_is(a[0], a[1], a[2], a[3], a[4], a[5], EPS_LO, EPS_HI, beta, cap, need_grad=False)
    assert none is None and torch.equal(out6.cpu(), out6b.cpu())
    dlogp, out6 = dlogp.cpu(), out6.cpu().to(F64)
    assert (dlogp[mask == 0] == 0).all()
    margin = 2 * _twin_worst()
    ratios = {"dlogp": _ratio((dlogp.to(F64) - r["dlogp"]).abs(), r["E"]),
              "loss": abs(out6[0].item() - r["loss"]) / r["E_loss"],
              "kl": abs(out6[1].item() - r["kl"]) / r["E_kl"] if beta else 0.0,
              "is_mean": abs(out6[3].item() - r["is_mean"]) / r["E_is"],
              "rollout_kl": abs(out6[5].item() - r["rollout_kl"]) / r["E_rkl"] if r["E_rkl"] > 0 else float(out6[5].item() != r["rollout_kl"])}
    print(f"\n[grpo-is] B{B} C{C} {'old' if use_old else 'noold'} beta{beta} cap{cap}: " + " ".join(f"{k_} {v_:.3f}" for k_, v_ in ratios.items())
          + f" (dlogp allowed {margin:.3f})")
    assert ratios["dlogp"] <= margin, ratios
    assert ratios["loss"] <= 1.0 and ratios["kl"] <= 1.0 and ratios["is_mean"] <= 1.0 and ratios["rollout_kl"] <= 1.0, ratios
    if not beta:
        assert out6[1].item() == 0.0
    # clip_ratio and is_capped: whole-number counts (exact in fp32) and one division
    assert abs(out6[2].item() - r["clip"]) <= 4 * U32 * max(r["clip"], 1e-30)
    assert abs(out6[4].item() - r["is_capped"]) <= 4 * U32 * max(r["is_capped"], 1e-30)
    assert 0.0 < out6[3].item() <= cap
    if cap == 1e30:
        assert out6[4].item() == 0.0
    if C > 1:
        assert 0.0 < r["is_capped"] < 1.0 or cap == 1e30     # (the inputs do put tokens on both sides of the cap)


@pytest.mark.parametrize("B,C,use_old,beta,cap", CASES)
def test_grpo_loss_is_equals_grpo_loss_on_policy(backend, B, C, use_old, beta, cap):
    """rollout_logp == q bit for bit: w = exp(0) = 1 exactly — out6[0..3) and dlogp are ops.grpo_loss's bits, is_mean 1, nothing capped,
    rollout_kl 0"""
    dev = backend
    lp, old, ref, adv, mask, _ = _inputs(B, C, use_old, cap)
    q = (old if old is not None else lp).clone()
    a = _dev_args(dev, lp, old, ref, adv, mask, q, beta)
    out3, d0 = ops.grpo_loss(a[0], a[1], a[2], a[3], a[4], EPS_LO, EPS_HI, beta)
    out6, d1 = ops.grpo_loss_is(a[0], a[1], a[2], a[3], a[4], a[5], EPS_LO, EPS_HI, beta, cap)
    assert torch.equal(d0.cpu().view(torch.int32), d1.cpu().view(torch.int32))
    assert torch.equal(out3.cpu().view(torch.int32), out6.cpu()[:3].view(torch.int32))
    assert out6[3].item() == 1.0 and out6[4].item() == 0.0 and out6[5].item() == 0.0


def test_grpo_loss_is_autograd_path(backend):
    """grpo.grpo_loss(rollout_logp=...): six statistics, the gradient is dlogp; without rollout_logp the three of before"""
    dev = backend
    lp, old, ref, adv, mask, rl = _inputs(4, 257, True, 2.0)
    r = _reference(lp, old, ref, adv, mask, rl, 0.04, 2.0)
    lpd = lp.to(dev).clone().requires_grad_(True)              # (a copy: on the CPU `.to` hands back the cached input itself)
    loss, stats = grpo.grpo_loss(lpd, old.to(dev), ref.to(dev), adv.to(dev), mask.to(dev), EPS_LO, EPS_HI, 0.04, rollout_logp=rl.to(dev), is_cap=2.0)
    assert stats.shape == (6,) and loss.item() == stats[0].item()
    loss.backward()
    assert _ratio((lpd.grad.cpu().to(F64) - r["dlogp"]).abs(), r["E"]) <= 2 * _twin_worst()
    loss3, stats3 = grpo.grpo_loss(lp.to(dev).clone().requires_grad_(True), old.to(dev), ref.to(dev), adv.to(dev), mask.to(dev), EPS_LO, EPS_HI, 0.04)
    assert stats3.shape == (3,)
    with pytest.raises(ValueError, match="is_cap"):
        grpo.grpo_loss(lpd, old.to(dev), ref.to(dev), adv.to(dev), mask.to(dev), EPS_LO, EPS_HI, 0.04, rollout_logp=rl.to(dev), is_cap=0.5)


def test_grpo_loss_is_refusals(backend):
    dev = backend
    lp, old, ref, adv, mask, rl = _inputs(4, 255, True, 2.0)
    a = _dev_args(dev, lp, old, ref, adv, mask, rl, 0.04)
    out6 = torch.full((6,), 77.0, dtype=F32, device=dev)
    dl = torch.full((4, 255), 77.0, dtype=F32, device=dev)

    def call(rl_, cap, B=4, C=255, lp_=a[0], out_=out6):
        with pytest.raises(KernelError) as ei:
            get_lib().call("bra_grpo_loss_is", lp_, a[1], a[2], a[3], a[4], rl_, B, C, EPS_LO, EPS_HI, 0.04, cap, out_, dl, current_stream(a[0]))
        assert (out6.cpu() == 77.0).all() and (dl.cpu() == 77.0).all()
        return ei.value.status

    assert call(None, 2.0) == BRA_ERR_ARG
    assert call(a[5], 0.999) == BRA_ERR_ARG
    assert call(a[5], 0.0) == BRA_ERR_ARG
    assert call(a[5], float("nan")) == BRA_ERR_ARG
    assert call(a[5], 2.0, B=0) == BRA_ERR_ARG
    assert call(a[5], 2.0, C=0) == BRA_ERR_ARG
    assert call(a[5], 2.0, lp_=None) == BRA_ERR_ARG
    assert call(a[5], 2.0, out_=None) == BRA_ERR_ARG
