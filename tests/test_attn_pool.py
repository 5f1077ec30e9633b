"""bra_attn_pool_fwd / bra_attn_pool_bwd (k_pool.hip) against a float64 statement of the formula, row by row.

    score[n, h, l] = x[n, l] . qt[h]  (valid keys only),  p = softmax_l(score),  pooled[n, h] = sum_l p[n, h, l] x[n, l]
    dqt[h] = d/dqt sum(pooled * g)

Criterion (the repository's standing one): for every (sequence, head) row of `pooled`, and every head row of `dqt`, the relative L2
error against float64 must be <= 1.25 x the error of the same formula evaluated in bf16 by torch on the CPU (x, qt cast to bf16)
against the same float64, the yardstick's error floored at its median over the rows.  Every row is compared.

The kernel walks a sequence in chunks of 128 rows per workgroup (kPoolTile in k_pool.hip; `chunk` = 0), so S = 387 spans three
whole chunks plus a 3-row tail; `chunk` = 256 makes one workgroup walk two tiles (the online-softmax rescale inside a chunk).
"""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NH = 8
CHUNK = 128


def formula(x, mask, qt, dtype):
    """-> pooled [n, 8, H] in `dtype`, qt leaf (for autograd)"""
    xx = x.to(dtype)
    q = qt.detach().to(dtype).clone().requires_grad_(True)
    s = torch.einsum("nld,hd->nhl", xx, q).masked_fill(mask[:, None, :] == 0, float("-inf"))
    return torch.einsum("nhl,nld->nhd", torch.softmax(s, dim=-1), xx), q


def row_err(a, truth):
    a, truth = a.detach().double().reshape(-1, a.shape[-1]), truth.detach().double().reshape(-1, truth.shape[-1])
    return (a - truth).norm(dim=1) / truth.norm(dim=1).clamp_min(1e-300)


def worst_ratio(ours, yard, truth, keep=None):
    """max over rows of err(ours) / max(err(yardstick), median err(yardstick))"""
    eo, ey = row_err(ours, truth), row_err(yard, truth)
    if keep is not None:
        eo, ey = eo[keep], ey[keep]
    return float((eo / ey.clamp_min(ey.median())).max())


def make_mask(kind, n, S):
    m = torch.ones(n, S, dtype=torch.uint8)
    if kind == "right":
        for i in range(n):
            m[i, max(1, S - 1 - (7 * i + S // 3) % S):] = 0
    elif kind == "left":                       # the first whole chunk (and a bit) masked
        for i in range(n):
            m[i, :min(S - 1, CHUNK + 12 + 5 * i)] = 0
    elif kind == "holes":
        g = torch.Generator().manual_seed(5)
        m = (torch.rand(n, S, generator=g) < 0.6).to(torch.uint8)
        m[:, S // 2] = 1
    elif kind == "one":
        m.zero_()
        for i in range(n):
            m[i, (S * (i + 1)) // (n + 1)] = 1
    elif kind == "none0":                      # row 0 has no valid key; the others are right-padded
        m = make_mask("right", n, S)
        m[0] = 0
    return m


def run_case(backend, n, S, H, kind="all", chunk=0, strided=False, scale_q=None, seed=0):
    from bioreason_amd import ops
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, S, H + (64 if strided else 0), generator=g).to(torch.bfloat16)[:, :, :H]
    qt = torch.randn(NH, H, generator=g) * (scale_q if scale_q is not None else 2.0 / H ** 0.5)
    go = torch.randn(n, NH, H, generator=g)
    mask = make_mask(kind, n, S)
    xd = x.to(backend)
    if strided:
        xd = torch.zeros(n, S, H + 64, dtype=torch.bfloat16, device=backend)[:, :, :H].copy_(x)
        assert xd.stride(1) == H + 64
    md, qd, gd = mask.to(backend), qt.to(backend), go.to(backend)
    pooled, lse = ops.attn_pool_fwd(xd, md, qd, chunk)
    dq = ops.attn_pool_bwd(xd, md, qd, pooled, lse, gd, chunk)
    pooled2, _ = ops.attn_pool_fwd(xd, md, qd, chunk)
    dq2 = ops.attn_pool_bwd(xd, md, qd, pooled, lse, gd, chunk)
    keep = mask.sum(1) > 0                                                     # sequences with a valid key
    assert torch.equal(pooled[keep.to(backend)], pooled2[keep.to(backend)]) and torch.equal(dq, dq2), "not bit-repeatable"
    out = {"x": x, "mask": mask, "pooled": pooled.cpu(), "lse": lse.cpu(), "dq": dq.cpu(), "keep": keep}
    # float64 truth and bf16 yardstick over the sequences that have a valid key (the others: NaN, checked by the caller)
    xs, ms, gs = x[keep], mask[keep], go[keep]
    pt, qleaf = formula(xs, ms, qt, torch.float64)
    (pt * gs.double()).sum().backward()
    py, qy = formula(xs, ms, qt, torch.bfloat16)
    (py * gs.to(torch.bfloat16)).sum().backward()
    if int(mask.sum(1).max()) == 1:
        # one valid key per sequence: p = 1, pooled is that row of x (the caller checks it bit for bit) and the true gradient is
        # exactly 0, so there is no relative error to take.  The kernel forms p (x . g' - pooled . g') with g' = g rounded to two bf16
        # halves; both dots are fp32 sums of the same H products in different orders, each within H 2^-24 sum|x g'| of the exact
        # value, so |dqt row| <= sum over sequences of 2 H 2^-24 sum_d |x_d g_d| |x|.
        xr = torch.stack([xs[i, int(ms[i].nonzero()[0, 0])] for i in range(xs.shape[0])]).double()          # [n, H]
        bound = (2 * H * 2.0 ** -24 * torch.einsum("nd,nhd->nh", xr.abs(), gs.double().abs()) * xr.norm(dim=1)[:, None]).sum(0)
        assert float(qleaf.grad.abs().max()) == 0.0
        print(f"attn_pool n={n} S={S} H={H} mask={kind}: |dqt| / bound {float((out['dq'].double().norm(dim=1) / bound).max()):.4f}")
        assert (out["dq"].double().norm(dim=1) <= bound).all()
        return out
    r_f = worst_ratio(out["pooled"][keep], py, pt)
    r_b = worst_ratio(out["dq"], qy.grad, qleaf.grad)
    print(f"attn_pool n={n} S={S} H={H} mask={kind} chunk={chunk}: worst ratio fwd {r_f:.4f} bwd {r_b:.4f}")
    assert torch.isfinite(out["pooled"][keep]).all() and torch.isfinite(out["dq"]).all()
    assert r_f <= 1.25, r_f
    assert r_b <= 1.25, r_b
    lse_t = torch.logsumexp(torch.einsum("nld,hd->nhl", xs.double(), qt.double()).masked_fill(ms[:, None, :] == 0, float("-inf")), -1)
    assert torch.allclose(out["lse"][keep].double(), lse_t, rtol=1e-4, atol=1e-3)
    return out


@pytest.mark.parametrize("H", [512, 768, 1024, 1920])
def test_hidden_sizes(backend, H):
    run_case(backend, 3, 130, H, "right")


@pytest.mark.parametrize("S", [1, 63, 64, 65])
def test_short_sequences(backend, S):
    out = run_case(backend, 1, S, 512, "all")
    if S == 1:
        assert torch.equal(out["pooled"][0], out["x"][0, 0].float().expand(NH, -1))


def test_three_chunks_and_a_tail(backend):
    assert 3 * CHUNK + 3 == 387
    run_case(backend, 5, 387, 512, "all")


def test_two_tiles_in_one_chunk(backend):
    run_case(backend, 2, 300, 512, "holes", chunk=256)


def test_strided_rows(backend):
    run_case(backend, 2, 130, 512, "right", strided=True)


@pytest.mark.parametrize("kind", ["right", "left", "holes"])
def test_masks(backend, kind):
    run_case(backend, 3, 387, 512, kind)


def test_one_valid_key_is_that_row_exactly(backend):
    out = run_case(backend, 3, 387, 512, "one")
    for i in range(3):
        row = int(out["mask"][i].nonzero()[0, 0])
        assert torch.equal(out["pooled"][i], out["x"][i, row].float().expand(NH, -1)), i


def test_sequence_without_a_valid_key_is_nan_and_alone(backend):
    out = run_case(backend, 3, 387, 512, "none0")           # rows 1, 2 went through the criterion in run_case
    assert torch.isnan(out["pooled"][0]).all()
    assert torch.isfinite(out["pooled"][1:]).all()


def test_large_scores_stay_finite(backend):
    H = 512
    out = run_case(backend, 3, 130, H, "right", scale_q=25.0 / H ** 0.5)
    assert out["lse"][out["keep"]].abs().max() > 60            # the scores do reach the range where exp() alone overflows fp32 sums


@pytest.mark.parametrize("H", [520, 4096])
def test_unsupported_hidden_sizes(backend, H):
    from bioreason_amd import _lib
    lib = _lib.get_lib()
    x = torch.zeros(1, 4, H, dtype=torch.bfloat16, device=backend)
    mask = torch.ones(1, 4, dtype=torch.uint8, device=backend)
    qt = torch.zeros(NH, H, device=backend)
    pooled, lse = torch.full((1, NH, H), 7.0, device=backend), torch.zeros(1, NH, device=backend)
    part, ml = torch.zeros(1, 1, NH, H, device=backend), torch.zeros(1, 1, NH, 2, device=backend)
    rc = lib.call_rc("bra_attn_pool_fwd", x, x.stride(0), x.stride(1), mask, qt, pooled, lse, part, ml, 1, 4, H, NH, 0, 0)
    assert rc == _lib.BRA_ERR_UNSUPPORTED
    rc = lib.call_rc("bra_attn_pool_bwd", x, x.stride(0), x.stride(1), mask, qt, pooled, lse, pooled, qt, part, 1, 4, H, NH, 0, 0)
    assert rc == _lib.BRA_ERR_UNSUPPORTED
    assert float(pooled.min()) == 7.0                          # nothing was launched
