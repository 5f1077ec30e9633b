"""The policy's entropy from the fused lm_head pass — ops.lmhead_logprob_entropy (EPI_LSE_ENT + bra_lse_ent_merge), ops.lmhead_dlogits
with ent / ecoef (EPI_DLOGIT_ENT), modeling._LogProbEntFn — row by row and element by element against float64 statements of the same
operations, by the convention of tests/test_loss_path_rowwise.py (read its docstring first; its operands, value sets, dispatch mirror
and fp32 terms F_lse, F_p are imported from it, not restated):

    err  <=  MARGIN[what] * E          E derived below, never fitted; MARGIN[what] = 2 x TWIN_WORST[what]

The references contain no project code: float64 logsumexp / softmax / autograd over h.double() @ e.double().T.

Notation: x_j the (bf16-rounded) logits of a row, m their maximum, a_j = x_j - m <= 0, s = sum_j exp(a_j), p_j = exp(a_j) / s,
A = sum_j p_j |a_j|, l_j = ln p_j = x_j - lse, H = -sum_j p_j l_j = ln s + A.  u = 2^-24, U = 2^-9.

ent.  The kernels form H = ln s - T / s, T = sum_c w_c (part_xs_c + (max_c - m) part_sum_c), w_c = exp(max_c - m); both terms >= 0.
  ln s     u (2 A + 8 + 3 |ln s|): F_lse of that module without its last addition m + ln s.
  T / s    every term of T is p_j a_j s.  Its exponentials carry u (2 |a_j| + 4) as in F_lse (the two products with log2 e, two ulps each
           of exp2); the factor x_j - max_c and the product with it 2 u; the rescale (max_c - m) part_sum_c, its sum with part_xs_c and the
           product with w_c 3 u; the additions that carry the row's mass 8 u as in F_lse; the division (a reciprocal and a product under
           -ffast-math) 3 u: u sum_j p_j |a_j| (2 |a_j| + 20); and s's own relative error u (2 A + 8) times T / s = A.
  the subtraction ln s - T / s rounds once: u H.
      F_H = u ( 2 A + 8 + 3 |ln s|  +  2 sum_j p_j a_j^2 + 20 A  +  A (2 A + 8)  +  H )
  Random sets add the first-order effect of rounding each logit (dH / dx_j = -p_j (l_j + H)):  U sum_j p_j |x_j| |l_j + H|.

dlogits, element (m, j):  ref = coef (1[j = tgt] - p_j) - ecoef p_j (l_j + H).  The bound of that module for the first term (with U |ref|
  for the whole element's bf16 rounding), plus  |ecoef| p_j ( |l_j + H| F_p + F_lse + F_H )  where F_p = u (2 + 3 |l_j|) + (the error of
  the lse fed), F_lse / F_H = the errors of the lse / ent fed (the kernels' own: E_lse / E_ent; the reference's rounded to fp32: u |lse|,
  u H), and that module's 2^-126 (1 + |coef|) for a flushed probability or element becomes 2^-126 (1 + |coef| + |ecoef| (1 + |l_j + H|)):
  a p_j below 2^-126 that the hardware flushes takes ecoef p_j (l_j + H) with it, |l_j + H| ~ 88 there.  (The kernel is left as it is:
  what the flush drops is below bf16's smallest normal number, 2^-126 times a few units, in a gradient whose row carries entries of
  order |coef|.)
  Random sets add the logit-rounding term of the entropy part, from
  d(-p_j (l_j + H)) / dx_k = -p_j ((1[j = k] - p_k) (l_j + H + 1) - p_k (l_k + H)):
      |ecoef| p_j U ( |l_j + H + 1| (|x_j| + sum_k p_k |x_k|) + sum_k p_k |x_k| |l_k + H| );  rows in the 2-norm.
  On the random sets the target element coef (1 - p_t) carries most of a row's 2-norm and the worst-case logit-rounding term allows
  about a percent on every p_j, so a common factor on the probabilities hides there; the same bound vector is therefore also held in
  the 1-norm against the row's SUM (sum_j dlogits[m, j] = coef (1[tgt >= 0] - sum p) - ecoef sum p (l + H): zero for a row with a
  target, whatever the logits): |sum_j err_j| <= sum_j E_j, with its own twin margin (`dl_sum`).
dh = gemm_nt(dlogits, E^T): that module's dh bound over the dlogits bound above.

The rounding twin: float64 logits rounded with .to(bfloat16), then a float32 torch restatement of the three 64-column partials in the
lanes' order, of the merge (lane = chunk, then the butterfly) and of the dlogits element, exp as exp2(a log2 e), log as log2(s) ln 2.
`test_twin_ratio_is_the_recorded_one` measures TWIN_WORST again on a CPU; `test_bounds_bite` corrupts the twin (never the kernel) five
ways and requires the check to reject each on an exact and on a random case.

Bit identity: logp / lse of lmhead_logprob_entropy and the three partial buffers it shares with bra_lmhead_lse_partials are torch.equal
to lmhead_logprob's on every case; lmhead_dlogits without ecoef is bra_lmhead_dlogits.
"""
import functools
import json
import math
import os
import sys
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bioreason_amd import ops, _lib                                    # noqa: E402
from test_loss_path_rowwise import (BF, F32, F64, U, U32, TINY, LOG2E, LN2, EXACT, PINNED, PINNED_SHAPES, _bf, _ratio, _exp32,      # noqa: E402
                                    _operands, _kernel, _lmhead_ref, _dh_kernels, edge_columns)

# The rounding twin's worst err / E per checked quantity over TWIN_CASES (CPU; test_twin_ratio_is_the_recorded_one measures them again)
TWIN_WORST = {
    "ent32": 0.39,      # exact sets (the fp32 term alone): 70x300x64-peaked
    "ent": 1.23,        # random sets: 330x300x64-rand (the pinned variants' shape)
    "dl_elem": 1.99,    # 130x1000x128-sparse: one bf16 rounding of the output, worst case 2 U, among 10^5 elements
    "dl_row": 1.01,     # 330x300x64-rand, fed the reference's lse / H (0.80 fed its own)
    "dl_sum": 0.15,     # 70x64x64-rand (random sets only: the row's sum in the 1-norm of the bound vector)
    "dh": 1.68,         # 330x1003x96-flat (dh = 0 in exact arithmetic: the rows of E are equal and a dlogits row sums to zero)
}
# 2 x the twin: the factor 2 is for what the twin does not model — the hardware's exp2 / log2, the MFMA accumulation order on the random
# sets, -ffast-math contraction
MARGIN = {k_: 2 * v_ for k_, v_ in TWIN_WORST.items()}
RATIO_FILE = os.path.join(os.environ.get("BRA_TEST_EVIDENCE_DIR") or os.path.join(ROOT, "test_evidence"), "lmhead_entropy_ratios.json")

# name: (M, V, K, values, option)   option: None | "strided" (h = a column slice of a wider tensor) | "notgt" (every fifth tgt = -1)
CASES = {}
for _M, _V, _K, _vals, _opt in [
    (70, 300, 64, "ints", None), (70, 300, 64, "ints", "strided"), (70, 300, 64, "sparse", None), (70, 300, 64, "peaked", None),
    (70, 300, 64, "flat", None), (70, 300, 64, "rand", None), (70, 300, 64, "big", "notgt"),
    (330, 301, 64, "sweep", None), (330, 301, 64, "big", None),
    (130, 1000, 128, "ints", "notgt"), (130, 1000, 128, "sparse", None), (130, 1000, 128, "rand", "notgt"), (130, 1000, 128, "big", "strided"),
    (330, 1003, 96, "sparse", None), (330, 1003, 96, "flat", None), (330, 1003, 96, "rand", None),
    (17, 65, 64, "peaked", None), (17, 65, 64, "flat", None), (17, 65, 64, "big", None),
    (70, 64, 64, "sweep", None), (70, 64, 64, "rand", None),
    (1, 64, 128, "ints", None), (1, 64, 128, "rand", None),
]:
    CASES[f"{_M}x{_V}x{_K}-{_vals}" + (f"-{_opt}" if _opt else "")] = (_M, _V, _K, _vals, _opt)
# the shapes at which the product library leaves the register-staged kernel (device only; see that module's docstring)
BIG_CASES = {"300x17700x64-ring": (300, 17700, 64, "ring"), "256x16400x64-glds256": (256, 16400, 64, "glds256"),
             "384x11100x64-glds192": (384, 11100, 64, "glds192"), "256x8200x64-glds128": (256, 8200, 64, "glds128")}


def _record(name, ratios, dev):
    if dev.type != "cuda":
        return
    os.makedirs(os.path.dirname(RATIO_FILE), exist_ok=True)
    try:
        with open(RATIO_FILE) as fh:
            data = json.load(fh)
    except (OSError, ValueError):
        data = {"margin": MARGIN, "twin_worst": TWIN_WORST, "cases": {}}
    data["cases"][name] = {k_: round(v_, 4) for k_, v_ in ratios.items()}
    with open(RATIO_FILE, "w") as fh:
        json.dump(data, fh, indent=1)


@functools.lru_cache(maxsize=None)
def _ecoef(M):
    """dL / d ent per row: both signs; rows 1, 15, 29, .. have coef = 0 too (`_operands`: coef[1::7] = 0) — all-zero rows — while rows 8,
    22, .. keep the entropy term alone; every eleventh row from 3 has the log-prob term alone"""
    g = torch.Generator().manual_seed(77 + M)
    ec = torch.randn(M, generator=g)
    ec[1::14] = 0
    ec[3::11] = 0
    if M == 1:
        ec[0] = 0.7
    return ec.to(F32)


# ----------------------------------------------------------------------------- float64 reference and bounds
def _ent_ref(h, e, tgt, coef, ecoef, exact):
    """that module's reference for the log-prob part, extended by the entropy: H, its bound, the dlogits of coef logp + ecoef H by
    float64 autograd, and the bound functions.  -> dict"""
    r = _lmhead_ref(h, e, tgt, coef, exact)
    x, lse, p = r["x"], r["lse"], r["p"]
    M, V = x.shape
    m = x.max(-1).values
    a = x - m[:, None]
    A = -(p * a).sum(-1)
    lns = lse - m
    l = x - lse[:, None]
    H = lns + A
    rb = 0.0 if exact else U
    f_H = U32 * (2 * A + 8 + 3 * lns.abs() + 2 * (p * a * a).sum(-1) + 20 * A + A * (2 * A + 8) + H)
    lH = l + H[:, None]
    spxl = (p * x.abs() * lH.abs()).sum(-1)
    r.update(H=H, E_ent=rb * spxl + f_H)
    # float64 autograd of sum_m (coef_m logp_m + ecoef_m H_m) with respect to the logits
    xg = x.detach().clone().requires_grad_(True)
    lsm = torch.log_softmax(xg, -1)
    has = tgt >= 0
    # (tgt = -1: logp = 0 - lse, that module's contract — the row has no one-hot)
    lp = torch.where(has, xg.gather(1, tgt.clamp(min=0).long()[:, None])[:, 0], torch.zeros_like(lse)) - torch.logsumexp(xg, -1)
    Hg = -(lsm.exp() * lsm).sum(-1)
    assert torch.allclose(Hg.detach(), H, rtol=0, atol=1e-11 * max(1.0, math.log(V)))
    (coef.to(F64) * lp + ecoef.to(F64) * Hg).sum().backward()
    dl = xg.grad
    c, ec = coef.to(F64)[:, None], ecoef.to(F64)[:, None]
    assert torch.allclose(dl, c * (r["onehot"] - p) - ec * p * lH, rtol=0, atol=1e-12 * (1 + c.abs().max().item() + ec.abs().max().item()) * max(1.0, math.log(V)))
    spx = (p * x.abs()).sum(-1)
    f_p = U32 * (2 + 3 * l.abs())
    r["dl"] = dl

    def dl_bound(lse_err, ent_err):
        """element bound of dlogits when the lse / ent it is fed are within lse_err / ent_err [M] of the row's"""
        Fp = f_p + lse_err[:, None]
        # (a probability below TINY may be flushed to zero: it takes coef p and ecoef p (l + H) with it, and the element itself may be)
        b = U * dl.abs() + c.abs() * p * (Fp + rb * (x.abs() + spx[:, None])) + TINY * (1 + c.abs() + ec.abs() * (1 + lH.abs()))
        b = b + ec.abs() * p * (lH.abs() * Fp + lse_err[:, None] + ent_err[:, None])
        if rb:
            b = b + ec.abs() * p * rb * ((lH + 1).abs() * (x.abs() + spx[:, None]) + spxl[:, None])
        return b

    r["dl_bound"] = dl_bound
    r["dh"] = dl @ e.to(F64)
    r["dh_bound"] = lambda b: U * r["dh"].abs() + (b + V * U32 * dl.abs()) @ e.to(F64).abs()
    return r


# ----------------------------------------------------------------------------- the rounding twin
def _lane_sum(t):
    """wave_sum of per-chunk terms t [M, nch]: lane = chunk mod 64 (sequential over c += 64), then the butterfly"""
    M, nch = t.shape
    lanes = torch.zeros(M, 64, dtype=F32, device=t.device)
    for c0 in range(0, nch, 64):
        blk = t[:, c0:c0 + 64]
        lanes[:, :blk.shape[1]] = lanes[:, :blk.shape[1]] + blk
    for half in (32, 16, 8, 4, 2, 1):
        lanes = lanes[:, :half] + lanes[:, half:2 * half]
    return lanes[:, 0]


def _partials32(xb):
    """float32 restatement of the EPI_LSE_ENT epilogue on logits xb [M, V]: per 64-column chunk the maximum, the sum of exp(x - max) and
    the sum of exp(x - max) (x - max), in the lanes' order (lane fq of a row holds columns 16 ni + 4 fq + r: 16 sequential additions, then
    the two cross-lane steps)"""
    M, V = xb.shape
    nch = -(-V // 64)
    x = torch.full((M, nch * 64), -math.inf, dtype=F32, device=xb.device)
    x[:, :V] = xb.to(F32)
    x = x.view(M, nch, 4, 4, 4)                                    # [chunk][ni][fq][r]
    cm = x.amax((2, 3, 4))
    d = x - cm[:, :, None, None, None]
    ex = torch.exp2(d * LOG2E)
    xe = torch.where(torch.isfinite(d), ex * d, torch.zeros_like(d))
    out = []
    for v in (ex, xe):
        v = v.permute(0, 1, 3, 2, 4).reshape(M, nch, 4, 16)
        acc = v[..., 0].clone()
        for i in range(1, 16):
            acc = acc + v[..., i]
        acc = acc + acc[..., [1, 0, 3, 2]]
        acc = acc + acc[..., [2, 3, 0, 1]]
        out.append(acc[..., 0])
    return cm, out[0], out[1]


def _merge32(cm, ps, px, corrupt=None):
    """float32 restatement of lse_ent_merge_kernel -> (lse, ent)"""
    if corrupt == "drop_xs":                                          # one chunk's part_xs dropped: the chunk of the row maximum
        px = px.clone()
        px.scatter_(1, cm.argmax(1, keepdim=True), 0.0)
    m = cm.amax(1)
    d = cm - m[:, None]
    w = torch.exp2(d * LOG2E)
    s = _lane_sum(ps * w)
    t = _lane_sum(w * (px + (0 if corrupt == "no_rescale" else d * ps)))
    ls = torch.log2(s) * LN2
    return m + ls, (ls - t / s).clamp_min(0.0)


def _twin(ref, tgt, coef, ecoef, e, corrupt=None):
    """(lse, ent, dlogits fed these, dlogits fed fp32(the reference's lse / H), dh) from the bf16-rounded float64 logits through the
    float32 restatement"""
    xb = _bf(ref["x"])
    lse, ent = _merge32(*_partials32(xb), corrupt)

    def dlogits(lse_, ent_):
        d = xb.to(F32) - lse_[:, None]
        p32 = _exp32(d) * (1.02 if corrupt == "p102" else 1.0)
        inner = d if corrupt == "no_ent" else d + ent_[:, None]
        sign = 1.0 if corrupt == "sign" else -1.0
        return (coef[:, None] * (ref["onehot"].to(F32) - p32) + sign * ecoef[:, None] * p32 * inner).to(BF)
    dl = dlogits(lse, ent)
    dh = (dl.to(F64) @ e.to(F64)).to(F32).to(BF)
    return lse, ent, dl, dlogits(ref["lse"].to(F32), ref["H"].to(F32)), dh


def _compare(ref, exact, ent, dl_own, dl_fed, dh, coef, ecoef):
    """worst ratios of the kernels' (or the twin's) results; dl_own: dlogits fed the same run's lse / ent, dl_fed: fed fp32(float64)"""
    out = {"ent32" if exact else "ent": _ratio((ent.to(F64) - ref["H"]).abs(), ref["E_ent"])}
    key = "dl_elem" if exact else "dl_row"
    for name, got, lse_err, ent_err in (("own", dl_own, ref["E_lse"], ref["E_ent"]), ("fed", dl_fed, U32 * ref["lse"].abs(), U32 * ref["H"])):
        if got is None:
            continue
        b = ref["dl_bound"](lse_err, ent_err)
        err = (got.to(F64) - ref["dl"]).abs()
        out[f"{key}_{name}"] = _ratio(err, b) if exact else _ratio(err.norm(dim=-1), b.norm(dim=-1))
        if not exact and name == "own":                             # the row's sum against the 1-norm of the same bound vector (with a consistent lse: sum p = 1)
            out[f"dl_sum_{name}"] = _ratio((got.to(F64).sum(-1) - ref["dl"].sum(-1)).abs(), b.sum(-1))
        zero = (coef == 0) & (ecoef == 0)
        assert (got[zero] == 0).all(), "a row with coef = 0 and ecoef = 0 must be exactly zero"
    if dh is not None:
        b = ref["dh_bound"](ref["dl_bound"](ref["E_lse"], ref["E_ent"]))
        out["dh"] = _ratio((dh.to(F64) - ref["dh"]).norm(dim=-1), b.norm(dim=-1))
    return out


def _passes(ratios):
    return all(v_ <= MARGIN[k_.rsplit("_", 1)[0] if k_.endswith(("_own", "_fed")) else k_] for k_, v_ in ratios.items())


def _assert_ratios(name, ratios, dev):
    print(f"\n[lmhead-entropy] {name}: " + " ".join(f"{k_} {v_:.3f}" for k_, v_ in ratios.items()))
    _record(name, ratios, dev)
    for k_, v_ in ratios.items():
        base = k_.rsplit("_", 1)[0] if k_.endswith(("_own", "_fed")) else k_
        assert v_ <= MARGIN[base], (name, k_, v_, MARGIN[base])


def _case_operands(M, V, K, vals, opt, dev, dom_cols=None):
    h0, e0, tgt0, coef0 = _operands(M, V, K, vals, dom_cols)
    tgt0 = tgt0.clone()
    if opt == "notgt":
        tgt0[::5] = -1
    h, e, tgt, coef, ecoef = h0.to(dev), e0.to(dev), tgt0.to(dev), coef0.to(dev), _ecoef(M).to(dev)
    if opt == "strided":
        wide = torch.full((M, K + 72), float("nan"), dtype=BF, device=dev)
        wide[:, 8:8 + K] = h
        h = wide[:, 8:8 + K]
        assert h.stride(0) != K
    return h, e, tgt, coef, ecoef


def _partials(lib, name, h, e, tgt, with_xs):
    M, K = h.shape
    V = e.shape[0]
    nch = -(-V // 64)
    bufs = [torch.full((M, nch), 7.0, dtype=F32, device=h.device) for _ in range(3 if with_xs else 2)]
    tl = torch.zeros(M, dtype=F32, device=h.device)
    lib.call(name, h, h.stride(0), e, e.stride(0), M, V, K, tgt, *bufs, tl, _lib.current_stream(h))
    return bufs, tl


def _run_case(name, dev, M, V, K, vals, opt, dom_cols=None, with_dh=True):
    exact = vals in EXACT
    h, e, tgt, coef, ecoef = _case_operands(M, V, K, vals, opt, dev, dom_cols)
    ref = _ent_ref(h, e, tgt, coef, ecoef, exact)
    if exact:
        assert torch.equal(_bf(ref["x"]), ref["x"]) and ref["x"].abs().max() <= 256      # every logit is a bf16 number
    if vals == "flat":
        assert torch.allclose(ref["H"], torch.full_like(ref["H"], math.log(V)), rtol=0, atol=1e-12)       # the closed form
    if vals == "peaked":
        assert (ref["H"] > 0).all() and (ref["H"] < 2e-3).all()
    # forward: the bits of lmhead_logprob, the three shared partial buffers included
    logp0, lse0 = ops.lmhead_logprob(h, e, tgt)
    logp, lse, ent = ops.lmhead_logprob_entropy(h, e, tgt)
    assert torch.equal(logp, logp0) and torch.equal(lse, lse0)
    lib = _lib.get_lib()
    (pm0, ps0), tl0 = _partials(lib, "bra_lmhead_lse_partials", h, e, tgt, False)
    (pm, ps, px), tl = _partials(lib, "bra_lmhead_lse_ent_partials", h, e, tgt, True)
    assert torch.equal(pm, pm0) and torch.equal(ps, ps0) and torch.equal(tl, tl0)
    assert (px <= 0).all()                                          # every term of part_xs is <= 0, every entry written
    assert (ent >= 0).all() and torch.isfinite(ent).all()
    dl_own = dl_fed = dh = None
    if V % 4 == 0:
        dl_own = ops.lmhead_dlogits(h, e, tgt, lse, coef, ent, ecoef)
        dl_fed = ops.lmhead_dlogits(h, e, tgt, ref["lse"].to(F32), coef, ref["H"].to(F32), ecoef)
        # without ecoef: today's entry point, bit for bit
        old = torch.empty((M, V), dtype=BF, device=dev)
        lib.call("bra_lmhead_dlogits", h, h.stride(0), e, e.stride(0), M, V, K, tgt, lse, coef, old, V, _lib.current_stream(h))
        assert torch.equal(ops.lmhead_dlogits(h, e, tgt, lse, coef), old)
        if with_dh:
            dh = _dh_kernels(dl_own, e)
    ratios = _compare(ref, exact, ent, dl_own, dl_fed, dh, coef, ecoef)
    _assert_ratios(name, ratios, dev)
    return ratios


# ----------------------------------------------------------------------------- 1 - 3: ent, bit identity, dlogits, dh
@pytest.mark.parametrize("name", list(CASES))
def test_lmhead_entropy_rowwise(backend, name):
    """ent per row; logp / lse / the shared partials bit for bit; dlogits with ent / ecoef per element (exact sets) / per row (random
    sets) fed its own and the reference's lse / ent; dh per row"""
    M, V, K, vals, opt = CASES[name]
    assert _kernel(M, V, K) == "nt128"
    _run_case(name, backend, M, V, K, vals, opt)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BIG_CASES))
def test_lmhead_entropy_product_dispatch(hip_device, name):
    """the ring and the LDS-DMA kernel as the product library dispatches them: exact logits, every row's dominant logit on an edge
    column of the first / last tiles"""
    M, V, K, kern = BIG_CASES[name]
    assert _kernel(M, V, K) == kern
    _run_case(name, hip_device, M, V, K, "sweep", None, dom_cols=tuple(edge_columns(V)), with_dh=False)


@pytest.mark.parametrize("variant", list(PINNED))
def test_lmhead_entropy_pinned_variants(debug_backend, variant):
    """both epilogue copies (gemm_epilogue; gemm_epilogue_w at MI = 2, 3, 4 and in the ring kernel)"""
    lib = _lib.get_lib()
    try:
        lib.call("bra_gemm_set_variant", variant)
        for (M, V, K) in PINNED_SHAPES:
            assert _kernel(M, V, K, variant) == PINNED[variant]
            for vals in ("sweep", "rand") if M >= V else ("ints", "big"):
                _run_case(f"v{variant}-{M}x{V}x{K}-{vals}", debug_backend, M, V, K, vals, None, with_dh=False)
    finally:
        lib.call("bra_gemm_set_variant", -1)


def test_dlogits_ent_argument_checks(backend):
    """ent without ecoef (or the reverse) is a ValueError; V % 4 != 0 and a missing ent / ecoef are BRA_ERR_ARG before any launch"""
    M, V, K = 17, 301, 64
    h, e, tgt, coef, ecoef = _case_operands(M, V, K, "ints", None, backend)
    _, lse, ent = ops.lmhead_logprob_entropy(h, e, tgt)
    with pytest.raises(ValueError):
        ops.lmhead_dlogits(h, e, tgt, lse, coef, ent=ent)
    with pytest.raises(ValueError):
        ops.lmhead_dlogits(h, e, tgt, lse, coef, ecoef=ecoef)
    with pytest.raises(_lib.KernelError) as ei:
        ops.lmhead_dlogits(h, e, tgt, lse, coef, ent, ecoef)
    assert ei.value.status == _lib.BRA_ERR_ARG
    out = torch.full((M, V), 3.0, dtype=BF, device=backend)
    st = _lib.current_stream(h)
    with pytest.raises(_lib.KernelError) as ei:
        _lib.get_lib().call("bra_lmhead_dlogits_ent", h, K, e, K, M, V, K, tgt, lse, coef, ent, ecoef, out, V, st)
    assert ei.value.status == _lib.BRA_ERR_ARG and (out.float() == 3.0).all()
    out4 = torch.full((M, 304), 3.0, dtype=BF, device=backend)
    for ent_, ecoef_ in ((None, ecoef), (ent, None)):
        with pytest.raises(_lib.KernelError) as ei:
            _lib.get_lib().call("bra_lmhead_dlogits_ent", h, K, e, K, M, V, K, tgt, lse, coef, ent_, ecoef_, out4, 304, st)
        assert ei.value.status == _lib.BRA_ERR_ARG and (out4.float() == 3.0).all()
    # the merge: logp may be null (lse and ent are written), part_xs may not
    (pm, ps, px), tl = _partials(_lib.get_lib(), "bra_lmhead_lse_ent_partials", h, e, tgt, True)
    lse2, ent2 = torch.empty_like(lse), torch.empty_like(ent)
    _lib.get_lib().call("bra_lse_ent_merge", pm, ps, px, None, lse2, None, ent2, M, pm.shape[1], st)
    assert torch.equal(lse2, lse) and torch.equal(ent2, ent)
    with pytest.raises(_lib.KernelError) as ei:
        _lib.get_lib().call("bra_lse_ent_merge", pm, ps, None, tl, lse2, None, ent2, M, pm.shape[1], st)
    assert ei.value.status == _lib.BRA_ERR_ARG


# ----------------------------------------------------------------------------- the twin, and that the bounds bite
TWIN_CASES = list(CASES) + [f"pinned-{M}x{V}x{K}-{vals}" for (M, V, K) in PINNED_SHAPES for vals in (("sweep", "rand") if M >= V else ("ints", "big"))]


def _twin_case(name):
    if name in CASES:
        M, V, K, vals, opt = CASES[name]
    else:
        M, V, K = (int(t) for t in name.split("-")[1].split("x"))
        vals, opt = name.split("-")[2], None
    h, e, tgt, coef = _operands(M, V, K, vals)
    if opt == "notgt":
        tgt = tgt.clone()
        tgt[::5] = -1
    return h, e, tgt, coef, _ecoef(M), vals in EXACT


def _twin_ratios(name, corrupt=None):
    h, e, tgt, coef, ecoef, exact = _twin_case(name)
    ref = _ent_ref(h, e, tgt, coef, ecoef, exact)
    lse, ent, dl, dl_fed, dh = _twin(ref, tgt, coef, ecoef, e, corrupt)
    return _compare(ref, exact, ent, dl, dl_fed, dh if corrupt is None else None, coef, ecoef)


def test_twin_ratio_is_the_recorded_one():
    """MARGIN's origin, reproducible without a GPU and without project code"""
    worst, where = dict.fromkeys(TWIN_WORST, 0.0), {}
    for name in TWIN_CASES:
        for k_, v_ in _twin_ratios(name).items():
            k_ = k_.replace("_own", "").replace("_fed", "")
            if v_ > worst[k_]:
                worst[k_], where[k_] = v_, name
    print(f"\n[lmhead-entropy] twin worst ratios {worst} at {where}")
    for k_ in TWIN_WORST:
        # (to the two digits written; the fp32-level one depends on the last bit of the host's exp2 / log2: two hundredths there)
        tol = 0.02 if k_ == "ent32" else 0.01
        assert math.isfinite(worst[k_]) and abs(worst[k_] - TWIN_WORST[k_]) <= tol, (k_, worst[k_], where.get(k_))
        assert MARGIN[k_] == 2 * TWIN_WORST[k_]


@pytest.mark.parametrize("corrupt", ["drop_xs", "no_rescale", "sign", "no_ent", "p102"])
def test_bounds_bite(corrupt):
    """each corruption of the TWIN is rejected by the check on at least one exact and at least one random case"""
    caught = {True: [], False: []}
    for name in CASES:
        exact = CASES[name][3] in EXACT
        if not _passes(_twin_ratios(name, corrupt)):
            caught[exact].append(name)
    print(f"\n[lmhead-entropy] {corrupt}: rejected on {len(caught[True])} exact and {len(caught[False])} random cases")
    assert caught[True] and caught[False], (corrupt, caught)


# ----------------------------------------------------------------------------- 5: modeling._LogProbEntFn
def _stub_model(e):
    eng = SimpleNamespace(E=e, ET=ops.transpose2d(e, pad_to=256), V=e.shape[0], ensure_transposed=lambda: None)
    return SimpleNamespace(engine=eng)


def test_logprob_ent_fn_backward(backend):
    """dh of sum(a logp) + sum(b ent) against float64 autograd, row by row (one dlogits launch, one gemm_nt); without the entropy term
    the backward takes _LogProbFn's dlogits call: its dh, bit for bit"""
    from bioreason_amd.modeling import _LogProbEntFn, _LogProbFn
    dev = backend
    M, V, K = 70, 320, 64
    h, e, tgt, a, b = _case_operands(M, V, K, "sparse", None, dev)
    model = _stub_model(e)
    calls = []
    real = ops.lmhead_dlogits

    def spy(*args, **kw):
        calls.append(len(args) + len(kw))
        return real(*args, **kw)
    ops.lmhead_dlogits = spy
    try:
        hg = h.clone().requires_grad_(True)
        logp, ent = _LogProbEntFn.apply(hg, model, tgt)
        ((a * logp).sum() + (b * ent).sum()).backward()
        assert calls == [7]                                         # ONE dlogits launch, with ent / ecoef
        h2 = h.clone().requires_grad_(True)
        logp2, ent2 = _LogProbEntFn.apply(h2, model, tgt)
        (a * logp2).sum().backward()                                # the entropy is a metric here: nobody differentiated it
        assert calls == [7, 5]
        h3 = h.clone().requires_grad_(True)
        logp3 = _LogProbFn.apply(h3, model, tgt)
        (a * logp3).sum().backward()
    finally:
        ops.lmhead_dlogits = real
    assert torch.equal(logp, logp3) and torch.equal(logp2, logp3) and torch.equal(ent, ent2)
    assert torch.equal(h2.grad, h3.grad)
    ref = _ent_ref(h, e, tgt, a, b, True)
    hd = h.to(F64).requires_grad_(True)
    lsm = torch.log_softmax(hd @ e.to(F64).T, -1)
    ((a.to(F64) * lsm.gather(1, tgt.long()[:, None])[:, 0]).sum() + (b.to(F64) * -(lsm.exp() * lsm).sum(-1)).sum()).backward()
    bound = ref["dh_bound"](ref["dl_bound"](ref["E_lse"], ref["E_ent"]))
    ratio = _ratio((hg.grad.to(F64) - hd.grad).norm(dim=-1), bound.norm(dim=-1))
    print(f"\n[lmhead-entropy] _LogProbEntFn dh {ratio:.3f}")
    _record("logprob_ent_fn", {"dh": ratio}, dev)
    assert ratio <= MARGIN["dh"]
    assert not torch.equal(hg.grad, h3.grad)                         # (the entropy term did reach dh)
