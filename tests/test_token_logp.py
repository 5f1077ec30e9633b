"""bra_token_logp (ops.token_logp) against float64, element by element: out[b, t] = logits[b, tok] - logsumexp(logits[b, :]) for the
token recorded at step t — the per-token log-probability the token loop reports under `return_logprobs`.

Criterion (the style of tests/test_loss_path_rowwise.py).  Every element is held to a first-order fp32 rounding bound

    E = ulp32(|x_tok|) + ulp32(|lse|) + D u,          u = 2^-24, ulp32(v) = 2^-23 |v|

  * ulp32(|lse|): lse = M + log(S) is formed in fp32 (M, the row maximum, is exact) — one rounding of a number of size |lse| — and
    the subtraction x_tok - lse rounds once more, to a result no larger than |x_tok| + |lse|: together below one ulp of each;
  * D u, the summation term: a relative error r on S = sum exp(x - M) is an absolute error r on log(S).  D counts the additions on
    the longest path of the kernel's fixed reduction tree — 4 EPT sequential additions per thread (EPT 16-byte groups of 4), 6
    butterfly steps of the wave, 4 wave partials, 6 butterfly steps over the 32 slices — plus 8 for the roundings every term carries
    whatever the tree: the subtraction x - M, the exponential (2 u), the slice rescale exp(M_s - M) and its product (3 u), the
    logarithm (2 u).

An fp32 torch twin of the same statement (m = max, s = sum exp(x - m), x_tok - (m + log s)) is measured against float64 on the same
inputs in the same test.  The allowed ratio is twice the twin's worst ratio over the input set: the twin cannot see the fast-exp
intrinsic (exp2(a log2 e): the product's rounding, 1.5 u |a| on the exponent) nor the kernel's summation order, and the factor 2 is
for those.  The measured ratios are printed (pytest -s) and recorded in NOTES.md.
"""
import functools
import math

import pytest
import torch

from bioreason_amd import ops
from bioreason_amd._lib import BRA_ERR_ARG, BRA_ERR_UNSUPPORTED, KernelError, current_stream, get_lib

F32, F64 = torch.float32, torch.float64
U32 = 2.0 ** -24
ROWS = 32                       # the input set of one V: 32 rows, kinds b % 8
T = 3                           # recorded steps; the kernel is run at the middle one
SENT = 123.0                    # what `out` holds where nothing may be written
LP_SLICES = 32                  # kLpSlices of k_grpo.hip


def _depth(V):
    per = (-(-V // LP_SLICES) + 3) // 4 * 4
    ept = -(-per // 1024)
    return 4 * ept + 6 + 4 + 6 + 8


@functools.lru_cache(maxsize=None)
def _inputs(V):
    """-> (logits fp32 [32, V], tokens int32 [32, T]); row kinds by b % 8:
    0 gaussian at Qwen3-like scale | 1 one logit 40 above the rest, drawn | 2 the same, NOT drawn (cancellation in x - lse: the drawn
    token's log-prob is about -40 - log V ... computed as a difference of numbers of size 40) | 3 flat | 4 the maximum in the last,
    partial slice | 5 the drawn token is the very last column | 6, 7 gaussian around -7 (every value negative)"""
    g = torch.Generator().manual_seed(7 * V + 1)
    x = torch.randn(ROWS, V, generator=g) * 3.0
    tok = torch.randint(0, V, (ROWS, T), generator=g, dtype=torch.int64)
    for b in range(ROWS):
        k = b % 8
        if k in (1, 2):
            d = int(tok[b, 1]) if k == 1 else (int(tok[b, 1]) + 1 + b) % V
            x[b, d] = x[b].max() + 40.0
        elif k == 3:
            x[b] = 1.25
        elif k == 4:
            x[b, V - 2 if V > 1 else 0] = x[b].max() + 10.0
        elif k == 5:
            tok[b, :] = V - 1
        elif k >= 6:
            x[b] = x[b] * (2.0 / 3.0) - 7.0
    return x.contiguous(), tok.to(torch.int32).contiguous()


@functools.lru_cache(maxsize=None)
def _reference(V, step):
    """float64 values, the bound E and the twin's worst ratio over the 32 rows — computed once per (V, step) and shared"""
    x, tok = _inputs(V)
    idx = tok[:, step].long()[:, None]
    x64 = x.to(F64)
    lse = torch.logsumexp(x64, dim=1)
    xt = x64.gather(1, idx)[:, 0]
    ref = xt - lse
    E = 2 * U32 * (xt.abs() + lse.abs()) + _depth(V) * U32
    m = x.max(dim=1, keepdim=True).values
    s = (x - m).exp().sum(dim=1)
    twin = x.gather(1, idx)[:, 0] - (m[:, 0] + s.log())
    assert twin.dtype == F32
    twin_ratio = ((twin.to(F64) - ref).abs() / E).max().item()
    return ref, E, twin_ratio


def _run(dev, V, B, pad, step, from_counter, x=None, tok=None):
    """rows 0 .. B-1 of the input set through the kernel at `step` -> out [B, T + 2] (pitch > T), everything else SENT"""
    if x is None:
        x, tok = _inputs(V)
    lg = torch.full((B, V + pad), -1.0e30 if pad else 0.0, dtype=F32)      # (pad columns: huge negatives a stray read would show as)
    lg[:, :V] = x[:B]
    lg = lg.to(dev)[:, :V]
    assert lg.stride(0) == V + pad
    out = torch.full((B, T + 2), SENT, dtype=F32, device=dev)
    st = torch.tensor([step], dtype=torch.int32, device=dev) if from_counter else step
    ops.token_logp(lg, tok[:B].to(dev).contiguous(), st, out[:, :T])
    return out.cpu()


CASES = [(V, B, pad, ctr) for V in (300, 4099, 151936) for B in (1, 8, 17, 32) for pad in (0, 24) for ctr in (False, True)]


@pytest.mark.parametrize("V,B,pad,from_counter", CASES)
def test_token_logp_vs_float64(backend, V, B, pad, from_counter):
    """V = 4099 is odd (rows 1, 2, ... are not 16-byte aligned at ldl = V, a ragged last group, a partial last slice); ldl = V and V + 24;
    the step from a device counter and from the argument; ldo = T + 2 > T, the middle column written, its neighbours untouched"""
    step = 1
    ref, E, twin_ratio = _reference(V, step)
    out = _run(backend, V, B, pad, step, from_counter)
    got = out[:, step].to(F64)
    ratio = ((got - ref[:B]).abs() / E[:B]).max().item()
    print(f"\n[token-logp] V={V} B={B} ldl=V+{pad} {'counter' if from_counter else 'arg'}: kernel {ratio:.4f} twin {twin_ratio:.4f} (allowed {2 * twin_ratio:.4f})")
    keep = torch.ones(T + 2, dtype=torch.bool)
    keep[step] = False
    assert (out[:, keep] == SENT).all(), "a column other than `step` was written"
    assert torch.isfinite(got).all()
    assert ratio <= 2 * twin_ratio, (ratio, twin_ratio)


@pytest.mark.parametrize("V", [32768, 32769, 163840, 163841, 262144])
def test_token_logp_slice_widths(backend, V):
    """the sizes at which the kernel changes its form: 1, 5 and 8 sixteen-byte groups per thread (slices of <= 1024, <= 5120, <= 8192
    columns), each boundary from both sides, and the largest vocabulary it takes"""
    g = torch.Generator().manual_seed(V)
    x = torch.randn(2, V, generator=g) * 3.0
    tok = torch.tensor([[5, V - 1, 0], [V // 2, 17, V - 1]], dtype=torch.int32)
    idx = tok[:, 1].long()[:, None]
    x64 = x.to(F64)
    lse = torch.logsumexp(x64, 1)
    ref = x64.gather(1, idx)[:, 0] - lse
    E = 2 * U32 * (x64.gather(1, idx)[:, 0].abs() + lse.abs()) + _depth(V) * U32
    m = x.max(1, keepdim=True).values
    twin = x.gather(1, idx)[:, 0] - (m[:, 0] + (x - m).exp().sum(1).log())
    twin_ratio = ((twin.to(F64) - ref).abs() / E).max().item()
    # (two elements: the twin's own worst over them can be luckily small — the input set of test_token_logp_vs_float64 at the
    #  production vocabulary is the yardstick for the allowed ratio here too)
    twin_ratio = max(twin_ratio, _reference(151936, 1)[2])
    out = _run(backend, V, 2, 0, 1, False, x=x, tok=tok)
    ratio = ((out[:, 1].to(F64) - ref).abs() / E).max().item()
    print(f"\n[token-logp] V={V} B=2: kernel {ratio:.4f} twin {twin_ratio:.4f}")
    assert ratio <= 2 * twin_ratio, (ratio, twin_ratio)


@pytest.mark.parametrize("V", [300, 4099, 151936])
def test_token_logp_row_does_not_depend_on_batch(backend, V):
    """row b of a B = 32 call equals row b of a B = b + 1 call bit for bit, from the counter and from the argument alike"""
    full = _run(backend, V, 32, 0, 1, False)[:, 1]
    assert torch.equal(full, _run(backend, V, 32, 0, 1, True)[:, 1])
    for b in (0, 7, 16, 31):
        part = _run(backend, V, b + 1, 0, 1, b % 2 == 0)[:, 1]
        assert torch.equal(part[b], full[b]), (V, b, part[b].item(), full[b].item())
        assert torch.equal(part, full[: b + 1])


def test_token_logp_every_step_of_a_matrix(backend):
    """the loop's use: one call per step fills the [B, T] matrix column by column; an id outside the vocabulary gives 0.0"""
    V, B = 4099, 8
    x, tok = _inputs(V)
    tok = tok[:B].clone()
    tok[3, 2] = V
    tok[4, 2] = -1
    dev = backend
    out = torch.full((B, T), SENT, dtype=F32, device=dev)
    ws = ops.token_logp_ws(B, dev)
    lg, tk = x[:B].to(dev), tok.to(dev)
    for t in range(T):
        ops.token_logp(lg, tk, t, out, ws)
    out = out.cpu()
    assert out[3, 2] == 0.0 and out[4, 2] == 0.0
    for t in range(T):
        ref, E, twin_ratio = _reference(V, t)
        ok = torch.ones(B, dtype=torch.bool)
        if t == 2:
            ok[3] = ok[4] = False
        assert (((out[:, t].to(F64) - ref[:B]).abs() / E[:B])[ok]).max().item() <= 2 * twin_ratio


def test_token_logp_refusals(backend):
    """every size the entry point refuses returns the error with the output untouched"""
    dev = backend
    V, B = 300, 4
    lg = torch.randn(B, V, dtype=F32).to(dev)
    tok = torch.zeros((B, T), dtype=torch.int32, device=dev)
    out = torch.full((B, T), SENT, dtype=F32, device=dev)
    ws = ops.token_logp_ws(64, dev)
    stp = torch.tensor([1], dtype=torch.int32, device=dev)

    def call(**kw):
        a = dict(logits=lg, ldl=V, B=B, V=V, tokens=tok, ldt=T, T=T, step_ptr=None, step=1, out=out, ldo=T, ws=ws)
        a.update(kw)
        with pytest.raises(KernelError) as ei:
            get_lib().call("bra_token_logp", a["logits"], a["ldl"], a["B"], a["V"], a["tokens"], a["ldt"], a["T"], a["step_ptr"], a["step"],
                           a["out"], a["ldo"], a["ws"], current_stream(lg))
        assert (out.cpu() == SENT).all()
        return ei.value.status

    assert call(B=0) == BRA_ERR_ARG
    assert call(B=-1) == BRA_ERR_ARG
    assert call(B=65) == BRA_ERR_UNSUPPORTED          # (refused on the sizes alone: nothing of the 65 rows is touched)
    assert call(V=0) == BRA_ERR_ARG
    assert call(V=262145, ldl=262145) == BRA_ERR_UNSUPPORTED
    assert call(ldl=V - 1) == BRA_ERR_ARG
    assert call(step=-1) == BRA_ERR_ARG
    assert call(step=T) == BRA_ERR_ARG
    assert call(T=0) == BRA_ERR_ARG
    assert call(ldt=T - 1) == BRA_ERR_ARG
    assert call(ldo=T - 1) == BRA_ERR_ARG
    for name in ("logits", "tokens", "out", "ws"):
        assert call(**{name: None}) == BRA_ERR_ARG
    # a device step outside [0, T) cannot be refused by the host: the kernel writes nothing
    for bad in (-1, T, 1 << 20):
        stp.fill_(bad)
        ops.token_logp(lg, tok, stp, out, ws)
        assert (out.cpu() == SENT).all()
    stp.fill_(1)
    ops.token_logp(lg, tok, stp, out, ws)
    o = out.cpu()
    assert (o[:, 1] != SENT).all() and (o[:, 0] == SENT).all() and (o[:, 2] == SENT).all()
