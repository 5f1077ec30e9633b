"""Everything between the GEMMs of a layer — k_norm.hip (RMSNorm forward / backward, LayerNorm, SwiGLU forward / backward, both kernel
families of per-head QK-norm + RoPE) and the tiled data movers of k_misc.hip — element by element against float64 statements of the
same operations.  tests/test_kernels.py bounds one Frobenius ratio per tensor of N(0, 1) values; here every element is held.

U = 2^-9 (half of bfloat16's worst-case relative rounding error), U32 = 2^-24 (fp32 unit roundoff), TINY = 2^-126 (the smallest normal
number).  The references contain no project code.

1. Forward kernels whose value is DEFINED by their rounding points (rmsnorm_fwd, swiglu_fwd, qk_norm_rope_fwd)

  The reference is a float64 twin with the roundings the kernel comments state:
      RMSNorm      bf16( w * bf16( x * rsqrt(mean x^2 + eps) ) )
      SwiGLU       bf16( bf16(silu(g)) * u )
      QK-norm+RoPE bf16(w * bf16(x * rstd)), then bf16(. * qscale) for q when qscale != 1, then the rotation with the fp32 table
                   entries taken exactly, one rounding; V copied bit for bit.
  Per element: got == twin bit for bit, or one bf16 ulp off — and that only where the float64 value v before SOME rounding of the
  element's chain lies within delta of a rounding boundary, bf16(v + delta) != bf16(v - delta), delta = tau |v| from the fp32 chain:
      rstd (row / head of n elements, a lane adds n_l of them in sequence, then log2(lanes) butterfly steps): the squares and their sum
        (n_l + steps + 1) u worst case (all terms positive), the division by n (a reciprocal, an ulp = 2 u, and a product under
        -ffast-math) and + eps: 4 u; the square root halves these; rsqrt itself an ulp: 2 u.
            tau_rstd = (n_l + steps + 5) / 2 + 2          [u]
      x * rstd: one product more, tau_in = tau_rstd + 1.   w * bf16(.) is a product of two 8-bit significands: exact in fp32, so the
        outer rounding flips only where the inner one did.  bf16(x * qscale): the fp32 product rounds once, tau = 1.
      silu(g) = g / (1 + e), e = __expf(-g) = exp2(-g log2 e): the product's rounding moves e by |g| u relatively, the constant's by
        half that, exp2 an ulp; (1 + e) carries e / (1 + e) of it and its own rounding, the division a reciprocal and a product:
            tau_silu = (1.5 |g| + 2) e / (1 + e) + 4      [u]        bf16(silu) * u is again exact in fp32.
      rotation o1 = x1 c - x2 s: two products and one addition, delta = u (|x1 c| + |x2 s| + |o1|) (absolute: the difference cancels);
        an inner rounding that is boundary-near marks both outputs of its pair.
  Flush: an output whose twin is below TINY in magnitude may be +-0.  SwiGLU: the chain's own intermediate 1 / (1 + e^-g) is below TINY for
  g < -87.34 (a reciprocal flushes it), and e^-g exceeds fp32 for -g > 128 ln 2 = 88.72: there the output may be +-0 too (and IS, from
  g = -89 on: asserted in the backward sweep).
  One ulp is all an inner flip can cost only while the outer product is exact in bf16 as well: the random SwiGLU forward cases take
  u = +-2^k for that reason (_swiglu_inputs), the sweep over every bf16 gate keeps a general u.
  What keeps the rule from hiding a failure: in every case the twin alone marks at most 1 % of the elements boundary-near (asserted).

2. Kernels with ONE output rounding of an fp32 expression (rmsnorm_bwd, layernorm_fwd, swiglu_bwd, qk_norm_rope_bwd)

  Reference: the unrounded float64 expression (autograd through the float64 forward without inner roundings, as the kernels
  differentiate).  Per element   err <= MARGIN[what] * E,   E = U |ref| + u (c * sum of the magnitudes of the added terms + R) + TINY:
    rmsnorm_bwd  dx = r (g - xh m) [+ dres], g = w dy (exact), xh = x r, m = mean(g xh).  r carries d_r = 4 + log2(n) / 2 [u] (rsqrt 2,
        division and eps 2, the sum of squares log2(n) halved); the first term d_r + 2 (subtraction, product), the second 2 d_r + 5:
        c = 13 + log2(n) on |r g| + |r xh m| + |dres|.   R = log2(n) mean|g xh| |xh| r: the dot's reduction.
    layernorm    y = (x - mean) r w + b.  mean: absolute error e_m = u (log2(n) + 3) mean|x|; d = x - mean: e_m + u |d|; the variance
        2 e_m mean|d| + u (log2(n) + 3) var, so r carries d_r = (that) / (2 (var + eps)) + 4 u.
        E = U |ref| + u 6 (|d r w| + |b|) + |r w| e_m + |d r w| d_r.   A constant row must be the bias bit for bit: that needs the mean of
        n equal values to be the value (the kernel corrects its reciprocal division by one fma step; without it 504 x 3.5 / 504 is an ulp
        off and eps = 1e-12 normalises that ulp to 0.2).
    swiglu_bwd   sg = 1 / (1 + e) carries tau_sg = (1.5 |g| + 2) e / (1 + e) + 4; du = d g sg: u |ref| (tau_sg + 2).
        dg = d u sg B, B = 1 + g (1 - sg): 1 - sg has the absolute error u (sg tau_sg + 2 (1 - sg)), so B u (|g| sg tau_sg + 2 |g| (1 - sg) + 2)
        and dg: u |d u| sg (|g| sg tau_sg + 2 |g| (1 - sg) + 2 + |B| (tau_sg + 3)).
    rope_bwd     g' = qscale R^T g: absolute error e_i = u (2 (|g1 c| + |g2 s|) + |g'|) qscale-scaled; without norm weights that is all.
        With: the RMSNorm backward per head on g', c = 13 + log2(hd), plus what e moves: r |w_i| e_i + r |xh_i| mean(|w| e |xh|).
  MARGIN = 2 x TWIN_WORST; TWIN_WORST is the worst err / E of a float32 torch restatement in the lanes' order (per lane in sequence, then a
  halving butterfly), measured on the CPU and measured again by test_twin_ratio_is_the_recorded_one.  The factor 2 covers what the twin
  does not model: the hardware's rsqrt and exp2 (an ulp each, not the CPU's), -ffast-math contraction and reciprocal divisions.
  Rows built to cancel (dy parallel to x / w with power-of-two weights: dx = r g eps r^2, six orders below its terms; dres = -bf16(dx))
  are held under their own key, `*32`: there the sum of magnitudes carries the bound, not |ref|.

3. The tiled movers (head_transpose, transpose2d, group_broadcast, gather_rows, scatter_rows, embed_scatter_fwd / bwd) bit for bit,
  padding exactly zero, sentinels around every destination untouched; group_sum (one rounding of an fp32 sum) against the float64
  sum with the boundary rule of part 1, delta = u (copies + 1) sum |terms| (0 where no partial sum can round), and with whole-number values for hard equality.

Worst ratios of every case go to layer_glue_rowwise_ratios.json in BRA_TEST_EVIDENCE_DIR (else test_evidence/), per backend.
"""
import functools
import json
import math
import os

import pytest
import torch

from bioreason_amd import ops, _lib

BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
U = 2.0 ** -9
U32 = 2.0 ** -24
TINY = 2.0 ** -126
NEAR_CAP = 0.01                # the only cap: share of elements the twin alone may mark boundary-near

# worst err / E of the float32 restatement over the cases of this module (CPU; test_twin_ratio_is_the_recorded_one measures them again).
# bf16's worst-case relative error is 2 U: an element-wise maximum over 10^5 elements sits just under 2 wherever U |ref| carries E.
TWIN_WORST = {
    "rms_bwd": 1.99,        # 3x2048 with dres: one bf16 rounding of the output, worst case 2 U
    "rms_bwd32": 1.04,      # the cancelling rows at 2048 columns: the fp32 terms alone (a lane adds 32 squares in sequence there)
    "ln": 1.97,             # 7x1280
    "swiglu_bwd": 1.99,     # the sweep over every bf16 gate value
    "rope_bwd": 1.99,       # hd 128, 2 x 2 heads, qscale without norm weights
}
MARGIN = {k_: 2 * v_ for k_, v_ in TWIN_WORST.items()}

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIO_FILE = os.path.join(os.environ.get("BRA_TEST_EVIDENCE_DIR") or os.path.join(ROOT, "test_evidence"), "layer_glue_rowwise_ratios.json")


# ----------------------------------------------------------------------------- helpers
def _f32(v):
    return float(torch.tensor(v, dtype=F32))


def _bf(x):
    return x.to(BF).to(F64)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _ord(t):
    """bf16 -> integers in value order (+0 and -0 both 0): the difference of two is their distance in ulps"""
    i = _bits(t).to(torch.int32) & 0xFFFF
    mag = i & 0x7FFF
    return torch.where((i & 0x8000) != 0, -mag, mag)


def _near(v, delta):
    """float64 v before a bf16 rounding lies within delta (absolute) of a rounding boundary"""
    return _bf(v + delta) != _bf(v - delta)


def _ratio(err, E):
    r = torch.where(E > 0, err / E.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return r.max().item() if r.numel() else 0.0


def _record(name, figures, dev):
    key = "device" if dev.type == "cuda" else "emulator"
    os.makedirs(os.path.dirname(RATIO_FILE), exist_ok=True)
    try:
        with open(RATIO_FILE) as fh:
            data = json.load(fh)
    except (OSError, ValueError):
        data = {}
    data["margin"], data["twin_worst"] = MARGIN, TWIN_WORST
    data.setdefault(key, {})[name] = {k_: (round(v_, 4) if isinstance(v_, float) else v_) for k_, v_ in figures.items()}
    with open(RATIO_FILE, "w") as fh:
        json.dump(data, fh, indent=1)


def _assert_rounded(name, got, pre, near, dev, flush=None):
    """part 1's criterion: got (bf16) against the twin's float64 value `pre` before the output rounding; `near`: the twin's own
    boundary-near mark; `flush`: where +-0 is a legal value besides (|twin| < TINY always is)"""
    got = got.detach().cpu()
    want = pre.to(BF)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    d = (_ord(got) - _ord(want)).abs()
    share = near.float().mean().item() if near.numel() else 0.0
    zero_ok = (pre.abs() < TINY) if flush is None else ((pre.abs() < TINY) | flush)
    ok = (d == 0) | ((d == 1) & near) | (zero_ok & (got.to(F64) == 0))
    fig = {"elements": d.numel(), "one_ulp_off": int(((d == 1) & near).sum()), "near_share": share, "bad": int((~ok).sum()), "max_ulps": int(d.max()) if d.numel() else 0}
    print(f"\n[layer-glue] {name}: " + " ".join(f"{k_} {v_}" for k_, v_ in fig.items()))
    _record(name, fig, dev)
    assert share <= NEAR_CAP, (name, share)
    assert not torch.isnan(got.float()).any(), name
    assert bool(ok.all()), (name, fig, torch.nonzero(~ok)[:8].tolist())


def _assert_ratios(name, ratios, dev):
    print(f"\n[layer-glue] {name}: " + " ".join(f"{k_} {v_:.3f}" for k_, v_ in ratios.items()))
    _record(name, ratios, dev)
    for k_, v_ in ratios.items():
        assert v_ <= MARGIN[k_], (name, k_, v_, MARGIN[k_])


def _lane_sum(v):
    """float32 sum over the last dim as one wave forms it: lane l takes elements 8 l .. 8 l + 7 of every 512-column round in sequence,
    then a halving butterfly over the 64 lanes"""
    rows, n = v.shape
    R = -(-n // 512)
    p = torch.zeros(rows, R * 512, dtype=F32)
    p[:, :n] = v
    p = p.view(rows, R, 64, 8)
    acc = torch.zeros(rows, 64, dtype=F32)
    for r in range(R):
        for i in range(8):
            acc = acc + p[:, r, :, i]
    for half in (32, 16, 8, 4, 2, 1):
        acc = acc[:, :half] + acc[:, half:2 * half]
    return acc                                                      # [rows, 1]


def _head_sum(v):
    """float32 sum over the last dim (a head) as the scalar RoPE kernels form it: pair (d, d + half), then a butterfly over half lanes"""
    half = v.shape[-1] // 2
    acc = v[..., :half] + v[..., half:]
    while acc.shape[-1] > 1:
        h = acc.shape[-1] // 2
        acc = acc[..., :h] + acc[..., h:]
    return acc


def _sentinel(shape, dev, val=-7.25):
    return torch.full(shape, val, dtype=BF, device=dev)


# ============================================================================= RMSNorm
RMS_COLS = [8, 64, 504, 512, 520, 1024, 2048, 2560, 4096]
RMS_ROWS = [1, 2, 3, 4, 5, 7, 9]
# every width with two row counts, every row count at least twice: a sparse cross
RMS_CASES = sorted({(RMS_ROWS[i % 7], c) for i, c in enumerate(RMS_COLS)} | {(RMS_ROWS[(i + 3) % 7], c) for i, c in enumerate(RMS_COLS)} | {(9, 520), (5, 4096), (4, 8)})
EPS = 1e-6


@functools.lru_cache(maxsize=None)
def _rms_inputs(rows, cols):
    """x [rows + 3, cols]: row scales 2^-20 .. 2^20 (mean x^2 below, near and above eps = 1e-6 ~ 2^-20), then an all-zero row, a row with
    one outlier 2^10 times the rest, a row at mean square ~ eps; w: N(0, 1) + sign flips, one zero, one negative for certain"""
    g = torch.Generator().manual_seed(31 * rows + cols)
    ex = torch.linspace(-20, 20, rows) if rows > 1 else torch.tensor([-10.0])
    x = torch.randn(rows + 3, cols, generator=g)
    x[:rows] *= (2.0 ** ex.round())[:, None]
    x[rows] = 0
    x[rows + 1, cols // 3] *= 2.0 ** 10
    x[rows + 2] *= 1e-3
    w = torch.randn(cols, generator=g) * 1.5
    w[0], w[cols // 2], w[cols - 1] = 0.0, -0.75, -2.5
    dy = torch.randn(rows + 3, cols, generator=g)
    dres = torch.randn(rows + 3, cols, generator=g)
    return x.to(BF), w.to(BF), dy.to(BF), dres.to(BF)


def _tau_rstd(n_l, steps):
    return (n_l + steps + 5) / 2 + 2


def _rms_fwd_twin(x, w, eps):
    xd = x.to(F64)
    cols = x.shape[-1]
    r = torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + _f32(eps))
    inner = xd * r
    tau = U32 * (_tau_rstd(8 * -(-cols // 512), 6) + 1)
    near = _near(inner, tau * inner.abs())
    return w.to(F64) * _bf(inner), near


def _rms_fwd_call(x, w, dev, pitched):
    """through ops.rmsnorm_fwd, or — pitched — x and y as column slices of wider buffers with sentinel pads and two guard rows"""
    rows, cols = x.shape
    if not pitched:
        return ops.rmsnorm_fwd(x.to(dev), w.to(dev), EPS)
    xw = torch.full((rows, cols + 24), float("nan"), dtype=BF, device=dev)
    xw[:, 8:8 + cols] = x.to(dev)
    yw = _sentinel((rows + 2, cols + 40), dev)
    xv, yv = xw[:, 8:8 + cols], yw[:rows, 16:16 + cols]
    _lib.get_lib().call("bra_rmsnorm_fwd", xv, xv.stride(0), w.to(dev), yv, yv.stride(0), None, rows, cols, EPS, _lib.current_stream(xv))
    out = yv.clone()
    yw[:rows, 16:16 + cols] = -7.25
    assert (yw.float() == -7.25).all(), "pad columns / guard rows written"
    return out


@pytest.mark.parametrize("rows,cols", RMS_CASES)
@pytest.mark.parametrize("pitched", [False, True])
def test_rmsnorm_fwd_every_element(backend, rows, cols, pitched):
    x, w, _, _ = _rms_inputs(rows, cols)
    pre, near = _rms_fwd_twin(x, w, EPS)
    ms = x.to(F64).pow(2).mean(-1)
    if rows >= 5:
        assert (ms[:rows] < EPS / 4).any() and (ms[:rows] > 4 * EPS).any()           # eps matters on some rows and not on others
    got = _rms_fwd_call(x, w, backend, pitched)
    assert (got[rows].float() == 0).all()                                            # the all-zero row: 0 * rsqrt(eps)
    _assert_rounded(f"rms_fwd-{rows}x{cols}" + ("-pitched" if pitched else ""), got, pre, near, backend)


def test_rmsnorm_refuses_ragged(backend):
    """cols % 8 != 0 or a pitch % 8 != 0: BRA_ERR_ARG before any launch, nothing written"""
    dev = backend
    for cols, ldx, ldy in ((12, 16, 16), (16, 20, 16), (16, 16, 20)):
        x = torch.ones(3, 24, dtype=BF, device=dev)
        y = _sentinel((3, 24), dev)
        w = torch.ones(24, dtype=BF, device=dev)
        with pytest.raises(_lib.KernelError) as ei:
            _lib.get_lib().call("bra_rmsnorm_fwd", x, ldx, w, y, ldy, None, 3, cols, EPS, _lib.current_stream(x))
        assert ei.value.status == _lib.BRA_ERR_ARG and (y.float() == -7.25).all()
        with pytest.raises(_lib.KernelError) as ei:
            _lib.get_lib().call("bra_rmsnorm_bwd", x, ldx, x, ldx, w, None, 0, y, ldy, 3, cols, EPS, _lib.current_stream(x))
        assert ei.value.status == _lib.BRA_ERR_ARG and (y.float() == -7.25).all()


def _rms_bwd_ref(dy, x, w, eps, dres):
    """float64 autograd through w * x * rsqrt(mean x^2 + eps) and the bound E of the module docstring"""
    n = x.shape[-1]
    xd = x.to(F64).requires_grad_(True)
    (w.to(F64) * xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + _f32(eps))).backward(dy.to(F64))
    ref = xd.grad
    xd = xd.detach()
    r = torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + _f32(eps))
    g, xh = w.to(F64) * dy.to(F64), xd * r
    m = (g * xh).mean(-1, keepdim=True)
    terms = (r * g).abs() + (r * xh * m).abs()
    if dres is not None:
        ref = ref + dres.to(F64)
        terms = terms + dres.to(F64).abs()
    L = math.log2(n)
    E = U * ref.abs() + U32 * ((13 + L) * terms + L * (g * xh).abs().mean(-1, keepdim=True) * xh.abs() * r) + TINY
    return ref, E


def _rms_bwd_twin(dy, x, w, eps, dres):
    xf, df, wf = x.to(F32), dy.to(F32), w.to(F32)
    n = x.shape[-1]
    ss, dot = _lane_sum(xf * xf), _lane_sum(wf * df * xf)
    r = torch.rsqrt(ss / n + torch.tensor(eps, dtype=F32))
    cm = dot * r / n
    o = r * (wf * df - xf * r * cm)
    if dres is not None:
        o = o + dres.to(F32)
    return o.to(BF)


def _rms_bwd_call(dy, x, w, dres, dev, pitched):
    rows, cols = x.shape
    if not pitched:
        return ops.rmsnorm_bwd(dy.to(dev), x.to(dev), w.to(dev), EPS, dres=dres.to(dev) if dres is not None else None)

    def wide(t, pad):
        b = torch.full((rows, cols + pad + 8), float("nan"), dtype=BF, device=dev)
        b[:, 8:8 + cols] = t.to(dev)
        return b[:, 8:8 + cols]
    dyv, xv = wide(dy, 8), wide(x, 16)
    dv = wide(dres, 24) if dres is not None else None
    ow = _sentinel((rows + 2, cols + 40), dev)
    ov = ow[:rows, 16:16 + cols]
    _lib.get_lib().call("bra_rmsnorm_bwd", dyv, dyv.stride(0), xv, xv.stride(0), w.to(dev), dv, dv.stride(0) if dv is not None else 0,
                        ov, ov.stride(0), rows, cols, EPS, _lib.current_stream(xv))
    out = ov.clone()
    ow[:rows, 16:16 + cols] = -7.25
    assert (ow.float() == -7.25).all(), "pad columns / guard rows written"
    return out


RMS_BWD_CASES = [(r_, c_, d_, p_) for i, (r_, c_) in enumerate(RMS_CASES) for d_, p_ in (((True, False), (False, True)) if i % 2 else ((False, False), (True, True)))]


def _rms_bwd_ratios(rows, cols, with_dres, run):
    x, w, dy, dres = _rms_inputs(rows, cols)
    ref, E = _rms_bwd_ref(dy, x, w, EPS, dres if with_dres else None)
    got = run(dy, x, w, dres if with_dres else None)
    return {"rms_bwd": _ratio((got.detach().cpu().to(F64) - ref).abs(), E)}


@pytest.mark.parametrize("rows,cols,with_dres,pitched", RMS_BWD_CASES)
def test_rmsnorm_bwd_every_element(backend, rows, cols, with_dres, pitched):
    ratios = _rms_bwd_ratios(rows, cols, with_dres, lambda dy, x, w, dres: _rms_bwd_call(dy, x, w, dres, backend, pitched))
    _assert_ratios(f"rms_bwd-{rows}x{cols}" + ("-dres" if with_dres else "") + ("-pitched" if pitched else ""), ratios, backend)


RMS_CANCEL_COLS = [64, 520, 2048, 4096]


@functools.lru_cache(maxsize=None)
def _rms_cancel_inputs(cols):
    """five rows whose dx cancels.  Rows 0-2: w = +-2^k and dy = 2^a x / w (exact in bf16): g = 2^a x, dx = r g (1 - r^2 mean x^2)
    = r g eps r^2 — at mean x^2 = 1 / 64 / 4096 that is 1e-6 .. 2e-10 of its two terms.  Rows 3-4: ordinary dy, dres = -bf16(dx)."""
    g = torch.Generator().manual_seed(cols)
    x = torch.randn(5, cols, generator=g) * torch.tensor([1.0, 8.0, 64.0, 1.0, 0.01])[:, None]
    w = (2.0 ** torch.randint(-2, 3, (cols,), generator=g).float()) * (torch.randint(0, 2, (cols,), generator=g).float() * 2 - 1)
    x, w = x.to(BF), w.to(BF)
    dy = torch.randn(5, cols, generator=g).to(BF)
    dy[:3] = (torch.tensor([1.0, 0.25, 2.0])[:, None] * x[:3].float() / w.float()).to(BF)
    assert torch.equal(dy[:3].to(F64) * w.to(F64), torch.tensor([1.0, 0.25, 2.0], dtype=F64)[:, None] * x[:3].to(F64))
    dx, _ = _rms_bwd_ref(dy, x, w, EPS, None)
    dres = torch.zeros(5, cols, dtype=BF)
    dres[3:] = (-dx[3:]).to(BF)
    return x, w, dy, dres


def _rms_cancel_ratios(cols, run):
    x, w, dy, dres = _rms_cancel_inputs(cols)
    ref, E = _rms_bwd_ref(dy, x, w, EPS, dres)
    r = torch.rsqrt(x.to(F64).pow(2).mean(-1, keepdim=True) + _f32(EPS))
    terms = (r * w.to(F64) * dy.to(F64)).abs()
    dx = _rms_bwd_ref(dy, x, w, EPS, None)[0]
    assert (ref[:3].abs() <= 4e-6 * terms[:3] + 1e-30).all() and (ref[3:].abs() <= 2 * U * dx[3:].abs() + 1e-30).all()      # they do cancel
    assert (U * ref[:3].abs() < 0.01 * E[:3]).all() and (U * ref[3:].abs() < 0.01 * U * dx[3:].abs() + 1e-30).all()      # |ref| carries nothing
    got = run(dy, x, w, dres)
    return {"rms_bwd32": _ratio((got.detach().cpu().to(F64) - ref).abs(), E)}


@pytest.mark.parametrize("cols", RMS_CANCEL_COLS)
def test_rmsnorm_bwd_cancelling_rows(backend, cols):
    ratios = _rms_cancel_ratios(cols, lambda dy, x, w, dres: _rms_bwd_call(dy, x, w, dres, backend, False))
    _assert_ratios(f"rms_bwd-cancel-{cols}", ratios, backend)


# ============================================================================= LayerNorm
LN_CASES = [(1, 504), (5, 512), (9, 520), (4, 1024), (7, 1280), (3, 8), (2, 64)]
LN_EPS = 1e-12


@functools.lru_cache(maxsize=None)
def _ln_inputs(rows, cols):
    """row scales 2^-10 .. 2^10, then a constant row (variance 0: y = b), a row with mean 1000 and spread 1 (bf16 holds 1000 +- 4 k)"""
    g = torch.Generator().manual_seed(17 * rows + cols)
    ex = torch.linspace(-10, 10, rows) if rows > 1 else torch.tensor([0.0])
    x = torch.randn(rows + 2, cols, generator=g)
    x[:rows] = x[:rows] * (2.0 ** ex.round())[:, None] + 0.5 * (2.0 ** ex.round())[:, None]
    x[rows] = 3.5
    x[rows + 1] += 1000.0
    w = torch.randn(cols, generator=g) * 1.5
    w[0], w[cols - 1] = 0.0, -2.0
    b = torch.randn(cols, generator=g)
    return x.to(BF), w.to(BF), b.to(BF)


def _ln_ref(x, w, b, eps):
    n = x.shape[-1]
    xd, wd, bd = x.to(F64), w.to(F64), b.to(F64)
    ref = torch.nn.functional.layer_norm(xd, (n,), wd, bd, _f32(eps))
    mean = xd.mean(-1, keepdim=True)
    d = xd - mean
    var = d.pow(2).mean(-1, keepdim=True)
    r = torch.rsqrt(var + _f32(eps))
    L = math.log2(n) + 3
    e_m = U32 * L * xd.abs().mean(-1, keepdim=True)
    d_r = (2 * e_m * d.abs().mean(-1, keepdim=True) + U32 * L * var) / (2 * (var + _f32(eps))) + 4 * U32
    e_d = e_m + U32 * d.abs()
    t = (d * r * wd).abs()
    E = U * ref.abs() + U32 * 6 * (t + bd.abs()) + (r * wd).abs() * e_d + t * d_r + TINY
    return ref, E


def _ln_twin(x, w, b, eps):
    xf, n = x.to(F32), x.shape[-1]
    mean = _lane_sum(xf) / n
    d = xf - mean
    r = torch.rsqrt(_lane_sum(d * d) / n + torch.tensor(eps, dtype=F32))
    return (d * r * w.to(F32) + b.to(F32)).to(BF)


def _ln_ratios(rows, cols, run):
    x, w, b = _ln_inputs(rows, cols)
    ref, E = _ln_ref(x, w, b, LN_EPS)
    got = run(x, w, b)
    return got, {"ln": _ratio((got.detach().cpu().to(F64) - ref).abs(), E)}


@pytest.mark.parametrize("rows,cols", LN_CASES)
def test_layernorm_every_element(backend, rows, cols):
    dev = backend
    got, ratios = _ln_ratios(rows, cols, lambda x, w, b: ops.layernorm_fwd(x.to(dev), w.to(dev), b.to(dev), LN_EPS))
    _, _, b = _ln_inputs(rows, cols)
    assert torch.equal(_bits(got[rows].cpu()), _bits(b)), "a constant row is the bias, bit for bit"
    _assert_ratios(f"ln-{rows}x{cols}", ratios, backend)


# ============================================================================= SwiGLU
def _sigmoid64(g):
    return 1.0 / (1.0 + torch.exp(-g))


def _tau_sg(g):
    e_share = 1.0 - _sigmoid64(g)                                    # e / (1 + e)
    return (1.5 * g.abs() + 2) * e_share + 4


def _swiglu_fwd_twin(gu):
    F = gu.shape[1] // 2
    g, u = gu[:, :F].to(F64), gu[:, F:].to(F64)
    silu = g * _sigmoid64(g)
    near = _near(silu, U32 * _tau_sg(g) * silu.abs())
    flush = _sigmoid64(g) < TINY
    return _bf(silu) * u, near, flush


@functools.lru_cache(maxsize=None)
def _sweep_g():
    """every finite bf16 value in [-100, 100], both signs (100 = 0x42C8)"""
    bits = torch.arange(0, 0x42C8 + 1, dtype=torch.int32).to(torch.int16).view(BF)
    return torch.cat([bits, -bits])


def _sweep_gu(uvals, dvals=None):
    """g = the sweep against every u (and d) value: gu [rows, 2 F] (and dact [rows, F]) with F = 1024, the tail padded with g = 0"""
    g = _sweep_g()
    combos = [(u_, d_) for u_ in uvals for d_ in (dvals or [1.0])]
    gg = g.repeat(len(combos))
    uu = torch.cat([torch.full((g.numel(),), u_, dtype=BF) for u_, _ in combos])
    dd = torch.cat([torch.full((g.numel(),), d_, dtype=BF) for _, d_ in combos])
    F = 1024
    rows = -(-gg.numel() // F)
    gu = torch.zeros(rows, 2 * F, dtype=BF)
    da = torch.zeros(rows, F, dtype=BF)
    flat = torch.zeros(rows * F, dtype=BF)
    flat[:gg.numel()] = gg
    gu[:, :F] = flat.view(rows, F)
    flat = torch.zeros(rows * F, dtype=BF)
    flat[:uu.numel()] = uu
    gu[:, F:] = flat.view(rows, F)
    flat = torch.zeros(rows * F, dtype=BF)
    flat[:dd.numel()] = dd
    da[:] = flat.view(rows, F)
    return gu, da


def test_swiglu_fwd_every_bf16_gate(backend):
    gu, _ = _sweep_gu([1.0, -1.0, 3.1415])
    pre, near, flush = _swiglu_fwd_twin(gu)
    got = ops.swiglu_fwd(gu.to(backend))
    _assert_rounded("swiglu_fwd-sweep", got, pre, near, backend, flush=flush)


@functools.lru_cache(maxsize=None)
def _swiglu_inputs(rows, F, pow2_u=False):
    """pow2_u (the forward cases): every u is +-2^k.  A boundary-near silu(g) may round the other way on another exp2 / reciprocal, an
    inner step of one ulp; times a general u that is 0.5 .. 2 ulps of the product and can round to TWO output ulps (measured on the
    device: g = 5.9375, silu 1.6 u below a boundary, u = 0.0732: 0.4355 against the twin's 0.4316).  With u a power of two the product
    is exact and an inner flip is exactly one output ulp, which is the criterion; the sweep keeps u = 3.1415 over every bf16 gate"""
    g = torch.Generator().manual_seed(rows * 7 + F + 1)
    gu = torch.randn(rows, 2 * F, generator=g)
    gu[:, :F] *= 2.0 ** torch.randint(-6, 6, (rows, F), generator=g).float()           # gates over 2^-6 .. 2^5 sigma
    dact = torch.randn(rows, F, generator=g)
    if pow2_u:
        u = gu[:, F:]
        gu[:, F:] = torch.sign(u) * 2.0 ** torch.log2(u.abs().clamp_min(2.0 ** -6)).round()
    return gu.to(BF), dact.to(BF)


SWIGLU_CASES = [(r_, F_, p_) for F_ in (8, 136, 6144, 9728) for r_ in (1, 9) for p_ in (False, True)]


def _swiglu_fwd_call(gu, dev, pitched):
    rows, F = gu.shape[0], gu.shape[1] // 2
    if not pitched:
        return ops.swiglu_fwd(gu.to(dev))
    gw = torch.full((rows, 2 * F + 24), float("nan"), dtype=BF, device=dev)
    gw[:, 8:8 + 2 * F] = gu.to(dev)
    aw = _sentinel((rows + 2, F + 40), dev)
    gv, av = gw[:, 8:8 + 2 * F], aw[:rows, 16:16 + F]
    _lib.get_lib().call("bra_swiglu_fwd", gv, gv.stride(0), av, av.stride(0), rows, F, _lib.current_stream(gv))
    out = av.clone()
    aw[:rows, 16:16 + F] = -7.25
    assert (aw.float() == -7.25).all(), "pad columns / guard rows written"
    return out


@pytest.mark.parametrize("rows,F,pitched", SWIGLU_CASES)
def test_swiglu_fwd_every_element(backend, rows, F, pitched):
    gu, _ = _swiglu_inputs(rows, F, pow2_u=True)
    pre, near, flush = _swiglu_fwd_twin(gu)
    _assert_rounded(f"swiglu_fwd-{rows}x{F}" + ("-pitched" if pitched else ""), _swiglu_fwd_call(gu, backend, pitched), pre, near, backend, flush=flush)


def test_swiglu_grid_stride_second_pass(backend):
    """1030 x 4096: rows F / 8 = 527 360 vectors > 2048 blocks x 256 threads, the grid-stride loop runs twice (forward and backward)"""
    rows, F = 1030, 4096
    assert rows * F // 8 > 2048 * 256
    gu, _ = _swiglu_inputs(rows, F, pow2_u=True)
    pre, near, flush = _swiglu_fwd_twin(gu)
    _assert_rounded("swiglu_fwd-1030x4096", ops.swiglu_fwd(gu.to(backend)), pre, near, backend, flush=flush)
    gu, dact = _swiglu_inputs(rows, F)
    got = ops.swiglu_bwd(gu.to(backend), dact.to(backend))
    # (gates reach -160 here: the flush rule of the backward sweep applies, _swiglu_bwd_check)
    _assert_ratios("swiglu_bwd-1030x4096", _swiglu_bwd_check("swiglu_bwd-1030x4096", gu, dact, got, backend), backend)


def _swiglu_bwd_ref(gu, dact):
    """float64 autograd of silu(g) u . d; -> (ref [rows, 2 F], E, sg)"""
    F = gu.shape[1] // 2
    x = gu.to(F64).requires_grad_(True)
    (torch.nn.functional.silu(x[:, :F]) * x[:, F:]).backward(dact.to(F64))
    ref = x.grad
    g, u, d = gu[:, :F].to(F64), gu[:, F:].to(F64), dact.to(F64)
    sg = _sigmoid64(g)
    tau = _tau_sg(g)
    B = 1 + g * (1 - sg)
    E_dg = U * ref[:, :F].abs() + U32 * (d * u).abs() * sg * (g.abs() * sg * tau + 2 * g.abs() * (1 - sg) + 2 + B.abs() * (tau + 3)) + TINY
    E_du = U * ref[:, F:].abs() + U32 * ref[:, F:].abs() * (tau + 2) + TINY
    return ref, torch.cat([E_dg, E_du], 1), sg


def _swiglu_bwd_twin(gu, dact):
    F = gu.shape[1] // 2
    g, u, d = gu[:, :F].to(F32), gu[:, F:].to(F32), dact.to(F32)
    sg = 1.0 / (1.0 + torch.exp2(-g * torch.tensor(1.4426950408889634, dtype=F32)))
    du = d * (g * sg)
    dg = d * u * (sg * (1.0 + g * (1.0 - sg)))
    return torch.cat([dg, du], 1).to(BF)


def _swiglu_bwd_check(name, gu, dact, got, dev, twin=False):
    """both halves separately; where the chain's sigmoid is below TINY an exact zero is legal, from g = -89 on (e^-g past fp32) it is due"""
    F = gu.shape[1] // 2
    ref, E, sg = _swiglu_bwd_ref(gu, dact)
    got = got.detach().cpu().to(F64)
    err = (got - ref).abs()
    flush = torch.cat([sg < TINY, sg < TINY], 1)
    err = torch.where(flush & (got == 0), torch.zeros_like(err), err)
    if not twin:
        due = torch.cat([gu[:, :F].to(F64) <= -89.0] * 2, 1)
        assert (got[due] == 0).all(), "g <= -89: e^-g overflows fp32, sg = 0, both halves exactly zero"
    r = {"dg": _ratio(err[:, :F], E[:, :F]), "du": _ratio(err[:, F:], E[:, F:])}
    print(f"\n[layer-glue] {name}: dg {r['dg']:.3f} du {r['du']:.3f}")
    return {"swiglu_bwd": max(r.values())}


def test_swiglu_bwd_every_bf16_gate(backend):
    gu, dact = _sweep_gu([1.0, -1.0, 3.1415], [1.0, -1.0, 3.1415])
    got = ops.swiglu_bwd(gu.to(backend), dact.to(backend))
    _assert_ratios("swiglu_bwd-sweep", _swiglu_bwd_check("swiglu_bwd-sweep", gu, dact, got, backend), backend)


def _swiglu_bwd_call(gu, dact, dev, pitched):
    rows, F = dact.shape
    if not pitched:
        return ops.swiglu_bwd(gu.to(dev), dact.to(dev))
    gw = torch.full((rows, 2 * F + 24), float("nan"), dtype=BF, device=dev)
    gw[:, 8:8 + 2 * F] = gu.to(dev)
    dw = torch.full((rows, F + 16), float("nan"), dtype=BF, device=dev)
    dw[:, 8:8 + F] = dact.to(dev)
    ow = _sentinel((rows + 2, 2 * F + 40), dev)
    gv, dv, ov = gw[:, 8:8 + 2 * F], dw[:, 8:8 + F], ow[:rows, 16:16 + 2 * F]
    _lib.get_lib().call("bra_swiglu_bwd", gv, gv.stride(0), dv, dv.stride(0), ov, ov.stride(0), rows, F, _lib.current_stream(gv))
    out = ov.clone()
    ow[:rows, 16:16 + 2 * F] = -7.25
    assert (ow.float() == -7.25).all(), "pad columns / guard rows written"
    return out


@pytest.mark.parametrize("rows,F,pitched", SWIGLU_CASES)
def test_swiglu_bwd_every_element(backend, rows, F, pitched):
    gu, dact = _swiglu_inputs(rows, F)
    got = _swiglu_bwd_call(gu, dact, backend, pitched)
    name = f"swiglu_bwd-{rows}x{F}" + ("-pitched" if pitched else "")
    _assert_ratios(name, _swiglu_bwd_check(name, gu, dact, got, backend), backend)


# ============================================================================= QK-norm + RoPE
NPOS, THETA = 4096, 1e6


@functools.lru_cache(maxsize=None)
def _rope_tables(hd):
    inv = 1.0 / (THETA ** (torch.arange(0, hd, 2, dtype=F64) / hd))
    fr = torch.arange(NPOS, dtype=F64)[:, None] * inv[None, :]
    return fr.cos().to(F32).contiguous(), fr.sin().to(F32).contiguous()


def _rope_pos(B, S):
    """per batch row: left-padded from 0 (five pad tokens at position 0), from 1000, ending at the last table row; further rows between"""
    rows = []
    for b in range(B):
        if b == 0:
            rows.append((torch.arange(S) - min(5, S - 1)).clamp_min(0))
        elif b == 1:
            rows.append(torch.arange(S) + 1000)
        elif b == 2:
            rows.append(torch.arange(S) + NPOS - S)
        else:
            rows.append(torch.arange(S) + 37 * b)
    return torch.stack(rows).to(torch.int32).reshape(-1)


# (hd, Hq, Hkv, norm, B, S, s_off)
ROPE_CASES = [
    (2, 4, 2, True, 3, 37, 0), (2, 1, 1, False, 3, 37, 5),
    (8, 2, 2, True, 3, 37, 5), (8, 4, 1, False, 3, 37, 0),
    (32, 4, 1, True, 3, 37, 5), (32, 2, 2, False, 3, 37, 0), (32, 1, 1, True, 4, 1, 5),
    (64, 4, 2, True, 3, 37, 5), (64, 2, 2, False, 3, 37, 0), (64, 1, 1, True, 3, 37, 0), (64, 4, 1, True, 5, 1, 5),
    (128, 4, 2, True, 3, 37, 0), (128, 2, 2, False, 3, 37, 5), (128, 1, 1, True, 3, 37, 5), (128, 4, 1, False, 3, 13, 0), (128, 4, 2, True, 4, 1, 5),
]
ROPE_RUNS = [c_ + (p_,) for c_ in ROPE_CASES for p_ in (("vec", "scalar") if c_[0] >= 64 else ("scalar",))]


def _rope_path(hd, q_token_stride):
    """which kernel bra_qk_norm_rope_* takes (k_norm.hip): the vector templates need hd 64 / 128 and every stride a multiple of 8"""
    return "vec" if hd in (64, 128) and q_token_stride % 8 == 0 else "scalar"


@functools.lru_cache(maxsize=None)
def _rope_inputs(hd, Hq, Hkv, norm, B, S):
    H, T = Hq + 2 * Hkv, B * S
    g = torch.Generator().manual_seed(1000 * hd + 10 * H + S)
    qkv = torch.randn(T, H * hd, generator=g) * torch.logspace(-3, 3, T)[:, None]          # eps = 1e-6 matters on the first tokens' heads
    qw = (torch.randn(hd, generator=g) * 1.2).to(BF) if norm else None
    kw = (1 + 0.4 * torch.randn(hd, generator=g)).to(BF) if norm else None
    if norm:
        qw[0] = -0.5
    dq = torch.randn(B, S, Hq, hd, generator=g).to(BF)
    dk = torch.randn(B, S, Hkv, hd, generator=g).to(BF)
    dv = torch.randn(B, S, Hkv, hd, generator=g).to(BF)
    return qkv.to(BF), qw, kw, _rope_pos(B, S), dq, dk, dv


def _qscale(hd, norm):
    return 1.0 if norm else hd ** -0.5


def _rope_fwd_twin(qkv, qw, kw, pos, B, S, Hq, Hkv, hd, qscale):
    """-> (q_pre, q_near, k_pre, k_near, v): float64 values before the output rounding and the twin's boundary-near marks"""
    cos, sin = _rope_tables(hd)
    half = hd // 2
    x = qkv.to(F64).view(B, S, Hq + 2 * Hkv, hd)
    p = pos.long().view(B, S)
    c, s = cos[p].to(F64)[:, :, None, :], sin[p].to(F64)[:, :, None, :]
    qs = _f32(qscale)

    def side(t, w, is_q):
        near = torch.zeros(t.shape, dtype=torch.bool)
        if w is not None:
            r = torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + _f32(EPS))
            inner = t * r
            tau = U32 * (_tau_rstd(8, max(1, int(math.log2(hd)))) + 1)
            near |= _near(inner, tau * inner.abs())
            t = _bf(w.to(F64) * _bf(inner))
        if is_q and qs != 1.0:
            pre = t * qs
            near |= _near(pre, U32 * pre.abs())
            t = _bf(pre)
        x1, x2 = t[..., :half], t[..., half:]
        o1, o2 = x1 * c - x2 * s, x2 * c + x1 * s
        nin = near[..., :half] | near[..., half:]
        n1 = _near(o1, U32 * ((x1 * c).abs() + (x2 * s).abs() + o1.abs())) | nin
        n2 = _near(o2, U32 * ((x2 * c).abs() + (x1 * s).abs() + o2.abs())) | nin
        return torch.cat([o1, o2], -1), torch.cat([n1, n2], -1)

    q, qn = side(x[:, :, :Hq], qw, True)
    k, kn = side(x[:, :, Hq:Hq + Hkv], kw, False)
    return q, qn, k, kn, x[:, :, Hq + Hkv:].to(BF)


def _q_view(B, S, Hq, hd, pad, dev, fill):
    """token-major [B, S, Hq, hd] view of a [B, S, Hq hd + pad] buffer (pad = 4: a token stride the vector kernels cannot take)"""
    buf = torch.full((B, S, Hq * hd + pad), fill, dtype=BF, device=dev)
    return buf, buf.as_strided((B, S, Hq, hd), (S * (Hq * hd + pad), Hq * hd + pad, hd, 1))


@pytest.mark.parametrize("hd,Hq,Hkv,norm,B,S,s_off,path", ROPE_RUNS)
def test_qk_norm_rope_fwd_every_element(backend, hd, Hq, Hkv, norm, B, S, s_off, path):
    dev = backend
    H, T = Hq + 2 * Hkv, B * S
    qkv, qw, kw, pos, _, _, _ = _rope_inputs(hd, Hq, Hkv, norm, B, S)
    qscale = _qscale(hd, norm)
    pad = 4 if (path == "scalar" and hd >= 64) else 0
    assert _rope_path(hd, Hq * hd + pad) == path
    if (H * hd // 2) % 256 and S > 1:
        assert (T * H * hd // 2) % 256 and (T * H * hd // 8) % 256          # the last block is ragged
    cos, sin = (t.to(dev) for t in _rope_tables(hd))
    qbuf, q = _q_view(B, S, Hq, hd, pad, dev, -7.25)
    tail = 2
    kc, vc = _sentinel((B, Hkv, s_off + S + tail, hd), dev), _sentinel((B, Hkv, s_off + S + tail, hd), dev, 5.5)
    to = lambda t: t.to(dev) if t is not None else None
    ops.qk_norm_rope_fwd(qkv.to(dev), to(qw), to(kw), cos, sin, pos.to(dev), S, Hq, Hkv, hd, EPS, qscale, q, kc.permute(0, 2, 1, 3), vc.permute(0, 2, 1, 3),
                         s_off=s_off)
    q_pre, q_near, k_pre, k_near, v = _rope_fwd_twin(qkv, qw, kw, pos, B, S, Hq, Hkv, hd, qscale)
    name = f"rope_fwd-hd{hd}-{Hq}x{Hkv}-{'norm' if norm else 'scale'}-B{B}S{S}-off{s_off}-{path}"
    if pad:
        assert (qbuf[:, :, Hq * hd:].float() == -7.25).all(), "q pad columns written"
    for cache, val in ((kc, -7.25), (vc, 5.5)):
        assert (cache[:, :, :s_off].float() == val).all() and (cache[:, :, s_off + S:].float() == val).all(), "cache rows outside the append written"
    assert torch.equal(_bits(vc[:, :, s_off:s_off + S].permute(0, 2, 1, 3).cpu()), _bits(v)), "V is a copy"
    _assert_rounded(name + "-q", q, q_pre, q_near, dev)
    _assert_rounded(name + "-k", kc[:, :, s_off:s_off + S].permute(0, 2, 1, 3), k_pre, k_near, dev)


def _rope_bwd_ref(qkv, qw, kw, pos, dq, dk, dv, B, S, Hq, Hkv, hd, qscale):
    """float64 autograd through the forward without inner roundings, and the bound E of the module docstring"""
    cos, sin = _rope_tables(hd)
    half, H = hd // 2, Hq + 2 * Hkv
    p = pos.long().view(B, S)
    c, s = cos[p].to(F64)[:, :, None, :], sin[p].to(F64)[:, :, None, :]
    qs, eps = _f32(qscale), _f32(EPS)
    xd = qkv.to(F64).view(B, S, H, hd).clone().requires_grad_(True)

    def fwd(t, w, scale):
        if w is not None:
            t = w.to(F64) * (t * torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + eps))
        t = t * scale
        x1, x2 = t[..., :half], t[..., half:]
        return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)

    out = (fwd(xd[:, :, :Hq], qw, qs) * dq.to(F64)).sum() + (fwd(xd[:, :, Hq:Hq + Hkv], kw, 1.0) * dk.to(F64)).sum() + (xd[:, :, Hq + Hkv:] * dv.to(F64)).sum()
    out.backward()
    ref = xd.grad
    xd = xd.detach()
    L = max(1.0, math.log2(hd))

    def bound(x, w, g, scale, r_):
        g1, g2 = g[..., :half], g[..., half:]
        gp = torch.cat([g1 * c + g2 * s, g2 * c - g1 * s], -1) * scale
        e = U32 * (2 * torch.cat([(g1 * c).abs() + (g2 * s).abs(), (g2 * c).abs() + (g1 * s).abs()], -1) * abs(scale) + gp.abs())
        if w is None:
            return U * r_.abs() + e + U32 * r_.abs() + TINY
        wd = w.to(F64)
        r = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
        xh = x * r
        gg = wd * gp
        m = (gg * xh).mean(-1, keepdim=True)
        terms = (r * gg).abs() + (r * xh * m).abs()
        moved = r * wd.abs() * e + r * xh.abs() * (wd.abs() * e * xh.abs()).mean(-1, keepdim=True)
        return U * r_.abs() + U32 * ((13 + L) * terms + L * (gg * xh).abs().mean(-1, keepdim=True) * xh.abs() * r) + moved + TINY

    E = torch.cat([bound(xd[:, :, :Hq], qw, dq.to(F64), qs, ref[:, :, :Hq]), bound(xd[:, :, Hq:Hq + Hkv], kw, dk.to(F64), 1.0, ref[:, :, Hq:Hq + Hkv]),
                   torch.zeros_like(ref[:, :, Hq + Hkv:])], 2)
    return ref.reshape(B * S, H * hd), E.reshape(B * S, H * hd)


def _rope_bwd_twin(qkv, qw, kw, pos, dq, dk, dv, B, S, Hq, Hkv, hd, qscale):
    cos, sin = _rope_tables(hd)
    half, H = hd // 2, Hq + 2 * Hkv
    p = pos.long().view(B, S)
    c, s = cos[p][:, :, None, :], sin[p][:, :, None, :]
    x = qkv.to(F32).view(B, S, H, hd)
    qs, eps = torch.tensor(qscale, dtype=F32), torch.tensor(EPS, dtype=F32)

    def side(x_, w, g, scale):
        g1, g2 = g[..., :half].to(F32), g[..., half:].to(F32)
        gp = torch.cat([g1 * c + g2 * s, g2 * c - g1 * s], -1)
        if scale is not None and float(scale) != 1.0:
            gp = gp * scale
        if w is None:
            return gp
        wf = w.to(F32)
        ss, dot = _head_sum(x_ * x_), _head_sum(wf * gp * x_)
        r = torch.rsqrt(ss / hd + eps)
        cm = dot * r / hd
        return r * (wf * gp - x_ * r * cm)

    out = torch.cat([side(x[:, :, :Hq], qw, dq, qs), side(x[:, :, Hq:Hq + Hkv], kw, dk, None), dv.to(F32)], 2)
    return out.to(BF).reshape(B * S, H * hd)


def _rope_bwd_ratio(got, ref, E, B, S, Hq, Hkv, hd):
    got = got.detach().cpu()
    nv = Hkv * hd
    err = (got.to(F64) - ref).abs()
    return {"rope_bwd": _ratio(err[:, :-nv], E[:, :-nv])}


@pytest.mark.parametrize("hd,Hq,Hkv,norm,B,S,s_off,path", ROPE_RUNS)
def test_qk_norm_rope_bwd_every_element(backend, hd, Hq, Hkv, norm, B, S, s_off, path):
    """dq a token-major view (padded by 4 on the scalar path at hd 64 / 128), dk / dv head-major (cache-layout) views"""
    dev = backend
    qkv, qw, kw, pos, dq, dk, dv = _rope_inputs(hd, Hq, Hkv, norm, B, S)
    qscale = _qscale(hd, norm)
    pad = 4 if (path == "scalar" and hd >= 64) else 0
    assert _rope_path(hd, Hq * hd + pad) == path
    cos, sin = (t.to(dev) for t in _rope_tables(hd))
    _, dqv = _q_view(B, S, Hq, hd, pad, dev, float("nan"))
    dqv.copy_(dq.to(dev))
    dkv = dk.to(dev).permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)            # [B, S, Hkv, hd] over head-major memory
    dvv = dv.to(dev).permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
    assert dkv.stride(2) == S * hd or S == 1 or Hkv == 1
    to = lambda t: t.to(dev) if t is not None else None
    got = ops.qk_norm_rope_bwd(qkv.to(dev), to(qw), to(kw), cos, sin, pos.to(dev), S, Hq, Hkv, hd, EPS, qscale, dqv, dkv, dvv)
    ref, E = _rope_bwd_ref(qkv, qw, kw, pos, dq, dk, dv, B, S, Hq, Hkv, hd, qscale)
    nv = Hkv * hd
    assert torch.equal(_bits(got.cpu()[:, -nv:]), _bits(dv.reshape(B * S, nv))), "dV passes through bit for bit"
    _assert_ratios(f"rope_bwd-hd{hd}-{Hq}x{Hkv}-{'norm' if norm else 'scale'}-B{B}S{S}-{path}", _rope_bwd_ratio(got, ref, E, B, S, Hq, Hkv, hd), dev)


def test_rope_cases_cover_both_paths():
    """every hd 64 / 128 case runs on both kernel families, the scalar one at butterfly spans of 32 and 64 lanes; decode-step calls
    (S = 1, T = B) and both cache offsets are among the cases"""
    for hd in (64, 128):
        assert {r_[-1] for r_ in ROPE_RUNS if r_[0] == hd} == {"vec", "scalar"}
    assert {r_[0] for r_ in ROPE_RUNS} == {2, 8, 32, 64, 128}
    assert {(r_[1], r_[2]) for r_ in ROPE_RUNS} == {(4, 2), (2, 2), (4, 1), (1, 1)}
    assert any(r_[5] == 1 for r_ in ROPE_RUNS) and {r_[6] for r_ in ROPE_RUNS} == {0, 5}
    assert all(r_[4] >= 3 for r_ in ROPE_RUNS)
    pos = _rope_pos(3, 37).view(3, 37)
    assert pos[0, 0] == 0 and pos[1, 0] == 1000 and pos[2, -1] == NPOS - 1 and not torch.equal(pos[0], pos[1])


# ============================================================================= the twin
def _twin_worst():
    worst, where = dict.fromkeys(TWIN_WORST, 0.0), {}

    def take(r, name):
        for k_, v_ in r.items():
            if v_ > worst[k_]:
                worst[k_], where[k_] = v_, name

    for rows, cols, with_dres, _ in RMS_BWD_CASES:
        take(_rms_bwd_ratios(rows, cols, with_dres, lambda dy, x, w, dres: _rms_bwd_twin(dy, x, w, EPS, dres)), f"rms_bwd-{rows}x{cols}-{with_dres}")
    for cols in RMS_CANCEL_COLS:
        take(_rms_cancel_ratios(cols, lambda dy, x, w, dres: _rms_bwd_twin(dy, x, w, EPS, dres)), f"cancel-{cols}")
    for rows, cols in LN_CASES:
        take(_ln_ratios(rows, cols, lambda x, w, b: _ln_twin(x, w, b, LN_EPS))[1], f"ln-{rows}x{cols}")
    gu, dact = _sweep_gu([1.0, -1.0, 3.1415], [1.0, -1.0, 3.1415])
    take(_swiglu_bwd_check("twin-sweep", gu, dact, _swiglu_bwd_twin(gu, dact), None, twin=True), "sweep")
    for rows, F, pitched in SWIGLU_CASES:
        if not pitched:
            gu, dact = _swiglu_inputs(rows, F)
            take(_swiglu_bwd_check(f"twin-{rows}x{F}", gu, dact, _swiglu_bwd_twin(gu, dact), None, twin=True), f"{rows}x{F}")
    for hd, Hq, Hkv, norm, B, S, _ in ROPE_CASES:
        qkv, qw, kw, pos, dq, dk, dv = _rope_inputs(hd, Hq, Hkv, norm, B, S)
        a = (qkv, qw, kw, pos, dq, dk, dv, B, S, Hq, Hkv, hd, _qscale(hd, norm))
        ref, E = _rope_bwd_ref(*a)
        take(_rope_bwd_ratio(_rope_bwd_twin(*a), ref, E, B, S, Hq, Hkv, hd), f"rope-hd{hd}-{Hq}x{Hkv}-{norm}-S{S}")
    return worst, where


def test_twin_ratio_is_the_recorded_one():
    """MARGIN's origin, reproducible without a GPU and without project code"""
    worst, where = _twin_worst()
    print(f"\n[layer-glue] twin worst ratios {worst} at {where}")
    _record("twin", worst, torch.device("cpu"))
    for k_ in TWIN_WORST:
        # (to the two digits written; the fp32-level one depends on the last bit of the host's exp2 / rsqrt: two hundredths there)
        tol = 0.02 if k_.endswith("32") else 0.01
        assert math.isfinite(worst[k_]) and abs(worst[k_] - TWIN_WORST[k_]) <= tol, (k_, worst[k_], where.get(k_))
        assert MARGIN[k_] == 2 * TWIN_WORST[k_]


# ============================================================================= the movers
def _randbits(shape, seed):
    """random finite bf16 bit patterns (both signs, every exponent but the top one)"""
    g = torch.Generator().manual_seed(seed)
    b = torch.randint(0, 0x7F80, shape, generator=g, dtype=torch.int32) | (torch.randint(0, 2, shape, generator=g, dtype=torch.int32) << 15)
    return b.to(torch.int16).view(BF)


@pytest.mark.parametrize("hd", [32, 64, 128])
@pytest.mark.parametrize("S", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("layout", ["token", "cache"])
def test_head_transpose_bits(backend, hd, S, layout):
    """[B, S, H, hd] -> [B, H, hd, pad64(S)]: bit for bit, columns S .. pad64(S) exactly zero although the source holds NaN beyond S"""
    dev = backend
    B, H, old = 2, 3, 3
    x = _randbits((B, S, H, hd), 100 * hd + S)
    if layout == "token":
        buf = torch.full((B, S + old, H, hd), float("nan"), dtype=BF, device=dev)
        buf[:, :S] = x.to(dev)
        view = buf[:, :S]
    else:
        buf = torch.full((B, H, S + old, hd), float("nan"), dtype=BF, device=dev)
        buf[:, :, :S] = x.to(dev).permute(0, 2, 1, 3)
        view = buf.permute(0, 2, 1, 3)[:, :S]
    out = ops.head_transpose(view).cpu()
    P = ops.pad64(S)
    assert out.shape == (B, H, hd, P)
    assert torch.equal(_bits(out[..., :S]), _bits(x.permute(0, 2, 3, 1)))
    assert (_bits(out[..., S:]) == 0).all(), "padding must be +0 bit patterns"


T2D = [1, 7, 8, 63, 64, 65, 100, 136]
T2D_CASES = sorted({(T2D[i], T2D[(i + k) % 8]) for i in range(8) for k in (0, 3, 5)} | {(65, 65), (136, 63), (63, 136)})


@pytest.mark.parametrize("rows,cols", T2D_CASES)
def test_transpose2d_bits(backend, rows, cols):
    """input a column slice of a wider buffer (NaN around it), pad_to 8 / 32 / 256: out[c, r] = in[r, c] bit for bit, pad columns zero"""
    dev = backend
    x = _randbits((rows, cols), 1000 * rows + cols)
    wide = torch.full((rows, (cols + 7) // 8 * 8 + 16), float("nan"), dtype=BF, device=dev)
    wide[:, 8:8 + cols] = x.to(dev)
    for pad_to in (8, 32, 256):
        out = ops.transpose2d(wide[:, 8:8 + cols], pad_to=pad_to).cpu()
        Rp = -(-rows // pad_to) * pad_to
        assert out.shape == (cols, Rp)
        assert torch.equal(_bits(out[:, :rows]), _bits(x.T))
        assert (_bits(out[:, rows:]) == 0).all()


GROUP_CASES = [(c_, a_, n_) for c_ in (1, 3, 8) for a_ in (False, True) for n_ in (8, 2056)]


@pytest.mark.parametrize("copies,with_add,n", GROUP_CASES)
def test_group_sum_every_element(backend, copies, with_add, n):
    """whole-number values: exact; random values: one rounding of the fp32 sum against the float64 sum under the boundary rule.
    Member stride n + 8; R n / 8 is no multiple of 256"""
    dev = backend
    R = 3
    assert (R * n // 8) % 256
    g = torch.Generator().manual_seed(copies * 10 + n)
    for kind in ("ints", "rand"):
        if kind == "ints":
            src = torch.randint(-16, 17, (R * copies, n), generator=g).float()
            add = torch.randint(-16, 17, (R, n), generator=g).float()
        else:
            # (same-signed members: a sum that cancels has delta / |sum| large, and the twin would mark more than the cap allows)
            src = torch.randn(R * copies, n, generator=g).abs() * 2.0 ** torch.randint(-14, 15, (R * copies, 1), generator=g).float()
            add = torch.randn(R, n, generator=g) * 0.25
        src, add = src.to(BF), add.to(BF)
        wide = torch.full((R * copies, n + 8), float("nan"), dtype=BF, device=dev)
        wide[:, :n] = src.to(dev)
        got = ops.group_sum(wide[:, :n], copies, add=add.to(dev) if with_add else None)
        terms = src.to(F64).view(R, copies, n)
        if with_add:
            terms = torch.cat([terms, add.to(F64)[:, None]], 1)
        pre, mags = terms.sum(1), terms.abs().sum(1)
        # every term is a multiple of q = the smallest ulp among them (bf16: 2^(e - 8) for |t| = m 2^e, m in [0.5, 1)); while the sum of the
        # magnitudes stays below 2^24 q, every partial sum in any order is a multiple of q that fp32 holds: no rounding before the last one
        ex = torch.where(terms != 0, torch.frexp(terms)[1], torch.full(terms.shape, 4096, dtype=torch.int32)).amin(1)
        exact = mags < torch.ldexp(torch.ones_like(mags), ex - 8 + 24)
        near = _near(pre, torch.where(exact, torch.zeros_like(mags), U32 * (copies + 1) * mags))
        name = f"group_sum-{copies}-{'add' if with_add else 'noadd'}-{n}-{kind}"
        if kind == "ints":
            assert torch.equal(_bf(pre), pre) and bool(exact.all()) and not bool(near.any())       # |sum| <= 9 * 16: a whole number that bf16 holds
        _assert_rounded(name, got, pre, near, dev)


@pytest.mark.parametrize("copies,n", [(c_, n_) for c_ in (1, 3, 8) for n_ in (8, 2056)])
def test_group_broadcast_bits(backend, copies, n):
    """src [R, I, s, hd] -> out[(r copies + c), i, :s] for every copy; the rows s .. N of every block (the gaps) keep their sentinel"""
    dev = backend
    R, I, hd = 3, 2, 8
    s = n // hd
    src = _randbits((R, I, s, hd), copies + n)
    out = _sentinel((R * copies, I, s + 2, hd), dev)
    ops.group_broadcast(src.to(dev), out, copies)
    out = out.cpu()
    want = src[:, None].expand(R, copies, I, s, hd).reshape(R * copies, I, s, hd)
    assert torch.equal(_bits(out[:, :, :s]), _bits(want))
    assert (out[:, :, s:].float() == -7.25).all()


@pytest.mark.parametrize("n,H", [(2100, 2048), (5, 8), (70, 136)])
def test_gather_scatter_embed_bits(backend, n, H):
    """2100 x 2048: n H / 8 = 537 600 vectors, past the 2048 x 256 grid — the grid-stride loops run twice; H = 8: one vector per row"""
    dev = backend
    g = torch.Generator().manual_seed(n + H)
    nsrc = n // 2 + 3
    x = _randbits((nsrc, H), n * 3 + H)
    rows = torch.randint(0, nsrc, (n,), generator=g).to(torch.int32)          # repeated source rows
    rows[0], rows[-1] = nsrc - 1, 0
    got = ops.gather_rows(rows.to(dev), x.to(dev)).cpu()
    assert torch.equal(_bits(got), _bits(x[rows.long()]))
    # scatter: unique destination rows in a taller output, the others stay zero
    y = _randbits((n, H), n * 5 + H)
    perm = torch.randperm(n + 7, generator=g)[:n].to(torch.int32)
    out = ops.scatter_rows(perm.to(dev), y.to(dev), n + 7).cpu()
    want = torch.zeros(n + 7, H, dtype=BF)
    want[perm.long()] = y
    assert torch.equal(_bits(out), _bits(want))
    # embed_scatter: tok_src all -1 (every row from the table), all >= 0 (every row a DNA row), mixed, and none
    V = 50
    emb, dna = _randbits((V, H), 7 * H + n), _randbits((nsrc, H), 11 * H + n)
    ids = torch.randint(0, V, (n,), generator=g).to(torch.int32)
    allsrc = torch.randint(0, nsrc, (n,), generator=g).to(torch.int32)
    mixed = torch.where(torch.rand(n, generator=g) < 0.5, allsrc, torch.full_like(allsrc, -1))
    for name, ts in (("none", None), ("minus", torch.full((n,), -1, dtype=torch.int32)), ("all", allsrc), ("mixed", mixed)):
        o = _sentinel((n + 1, H), dev)
        ops.embed_scatter_fwd(ids.to(dev), ts.to(dev) if ts is not None else None, emb.to(dev), dna.to(dev), o[:n])
        want = emb[ids.long()]
        if ts is not None:
            want = torch.where((ts >= 0)[:, None], dna[ts.clamp_min(0).long()], want)
        assert torch.equal(_bits(o[:n].cpu()), _bits(want)), name
        assert (o[n].float() == -7.25).all(), name
    # backward: unique DNA rows receive their token's gradient, rows nobody references stay zero, tokens with -1 send nothing
    uniq = torch.full((n,), -1, dtype=torch.int32)
    k = min(n, nsrc) // 2 + 1
    uniq[torch.randperm(n, generator=g)[:k]] = torch.randperm(nsrc, generator=g)[:k].to(torch.int32)
    dout = _randbits((n, H), 13 * H + n)
    ddna = ops.embed_scatter_bwd(uniq.to(dev), dout.to(dev), torch.zeros(nsrc, H, dtype=BF, device=dev)).cpu()
    want = torch.zeros(nsrc, H, dtype=BF)
    want[uniq[uniq >= 0].long()] = dout[uniq >= 0]
    assert torch.equal(_bits(ddna), _bits(want))
