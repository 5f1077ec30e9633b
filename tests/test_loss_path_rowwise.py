"""The loss path — lmhead_logprob -> grpo_loss -> lmhead_dlogits -> gemm_nt(dlogits, E^T) — and the GRPO bookkeeping kernels of
k_grpo.hip, row by row and column by column against float64 statements of the same operations.

tests/test_kernels.py bounds one Frobenius ratio over a whole [M, V] tensor.  The target column coef (1 - p_t) carries most of a
dlogits row's norm, so every softmax probability times 1.02 passes there; a column dropped from one 64-column chunk, a one-hot on the
neighbouring column, a `chunk` index off by one move a handful of rows.  Here every row (every element, where the logits are exact)
is held against its own first-order rounding bound:

    err  <=  MARGIN[what] * E          E derived below, never fitted; MARGIN[what] = 2 x TWIN_WORST[what]

The references contain no project code: float64 logsumexp / softmax / autograd over h.double() @ e.double().T, and
oracle/grpo_math.py (the trainer's statements, pinned by tests/test_oracle_pinned.py) in float64 for the GRPO kernels.

The lm_head kernels round every logit to bf16 before the softmax (round_bf(acc) in both epilogue copies of k_gemm.hip), so there are
two kinds of value set:

  exact   h, e small integers with K |h| |e| <= 256: every logit is a whole number that bf16 holds — no accumulation order can flip a
          rounding, and lse / logp / dlogits are held at fp32 level.  `ints`, `sparse` (flat softmax: every column carries mass),
          `sweep` (row i's dominant logit, 128, on column i mod V: every column carries some row's whole mass), `peaked` (p_t >=
          1 - 1e-4 on the placed targets: the 1 - exp(x_t - lse) cancellation), `flat` (all logits equal: lse = x + ln V).
  random  N(0, s) bf16 operands (`rand`: the scale of tests/test_kernels.py; `big`: |logit| up to about 30).  The reference keeps the
          unrounded logits; the bound adds the first-order effect of rounding each logit x_j to bf16, relative U = 2^-9:
              lse:   U sum_j p_j |x_j|           logp:  U (|x_t| + sum_j p_j |x_j|)

The fp32 term (u = 2^-24, m = the row maximum, s = sum_j exp(x_j - m)):
    F_lse  = u ( 2 sum_j p_j |x_j - m|  +  8  +  3 |ln s|  +  |lse| )
  __expf is exp2 of the fp32 product a log2(e): the product's rounding moves the result by u |a| relatively, the constant's by half
  that, and a = x - chunk max, chunk max - m add up to x - m (first term);  8 = the two exponentials' own ulp (2 u each), the product
  partial sum x exp, and the three or so additions that carry a row's mass;  __logf is log2(s) ln 2 (an ulp of the result and the
  product: 3 u |ln s|);  the last addition m + ln s rounds once (u |lse|).   F_logp = F_lse + u |logp|.
  p_j as the dlogits epilogue forms it, exp(x_j - lse): relative error  F_p = u (2 + 3 |x_j - lse|) + (the error of the lse it was fed).

dlogits, element (m, j):   U |ref| + |coef| p_j F_p + 2^-126 (1 + |coef|)   [+ |coef| p_j U (|x_j| + sum p |x|) on the random sets];  rows in the 2-norm of that
  vector on the random sets.  For `peaked` the fp32 term dominates: ref = coef (1 - p_t) is 1e-6 .. 1e-4 |coef| while p_t F_p ~ u |lse|.
dh = gemm_nt(dlogits, E^T):  U |dh| + (the dlogits bound vector + V u |dlogits|) |E|, rows in the 2-norm.

The rounding twin (no project code): float64 logits rounded with .to(bfloat16), then a float32 torch restatement of the 64-column
partial maximum / sum (in the lanes' order) and of the merge, exp as exp2(a log2 e), bf16 dlogits, bf16 dh.
`test_twin_ratio_is_the_recorded_one` measures TWIN_WORST again on a CPU.

Dispatch.  `_kernel` restates pick_variant / pick_glds_rows / launch_gemm / dispatch_bk (k_gemm.hip) for the two lm_head entry points
(no LoRA pair, no split-K; the four-wave kernel has no LSE / dlogits epilogue).  What the product library can reach and who takes it:

    nt128   register-staged 128 x 128 tiles, gemm_epilogue          every small shape of this module (K = 96: the BK = 32 instance)
    ring    256 x 256 ring kernel, gemm_epilogue_w<8>               300 x 17700 x 64 (140 tiles), device only
    glds256 LDS-DMA 256 x 128 tiles, gemm_epilogue_w<4>             256 x 16400 x 64 (129 tiles; 65 ring tiles are too few), device only
    glds192 LDS-DMA 192 x 128 tiles, gemm_epilogue_w<3>             384 x 11100 x 64 (174 tiles in one round; 261 of 128 rows need two), device only
    glds128 LDS-DMA 128 x 128 tiles, gemm_epilogue_w<2>             256 x 8200 x 64 (130 tiles of 128 x 128; 65 of 256 rows are too few), device only
  Pinned with bra_gemm_set_variant on the
  debug library / the emulator: 0 (nt128), 2 (nt256, same epilogue at four row-waves), 5 / 9 / 10 (LDS-DMA at 256 / 192 / 128 rows:
  gemm_epilogue_w at MI = 4 / 3 / 2), 6 (ring).

Contracts stated and asserted here:
  tgt[m] = -1 (GemmArgs: "target column per row (or -1)"): bra_lmhead_lse_partials leaves tgt_logit[m] as the caller set it and the
  row's partials are complete; ops.lmhead_logprob hands in zeros, so lse is the row's and logp = 0 - lse.  In dlogits the row has no
  one-hot: coef (0 - p).
  V % 4 != 0: ops.lmhead_dlogits writes rows of pitch V, which bra_lmhead_dlogits refuses (ldd % 4, BRA_ERR_ARG) before any launch.
  gemm_nt contracts over V and needs V % 32 == 0 (Qwen3's 151 936 is): for the other V the test copies dlogits into a zero-padded
  buffer of the next multiple of 32 and uses E^T padded likewise; at V = 64 / 128 it takes the ET[:, :V] slice of a wider E^T.
"""
import functools
import json
import math
import os

import pytest
import torch

from bioreason_amd import ops, _lib
from oracle import grpo_math

BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
U = 2.0 ** -9                  # as in tests/test_attn_rowwise.py: half of bfloat16's worst-case relative rounding error
U32 = 2.0 ** -24               # fp32 unit roundoff
TINY = 2.0 ** -126             # the smallest normal fp32 / bf16 number: a probability or a product below it may be flushed to zero
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453

# The rounding twin's worst err / E per checked quantity over TWIN_CASES (CPU; test_twin_ratio_is_the_recorded_one measures them again)
# and where each was reached.  bf16's worst-case relative error is 2 U, so an element-wise maximum over 10^5 elements sits just under 2.
TWIN_WORST = {
    "lse32": 0.74,      # exact sets (the fp32 term alone): 70x300x96-ints-strided
    "logp32": 0.76,     # 257x520x128-ints
    "lse": 1.78,        # random sets: 257x520x128-big (a row whose mass sits on two or three logits, each rounded nearly 2 U off)
    "logp": 1.68,       # the same case
    "dl_elem": 1.99,    # 130x1000x64-ints-notgt: one bf16 rounding of the output, worst case 2 U, among 10^5 elements
    "dl_row": 1.02,     # 330x300x64-rand
    "dh": 1.60,         # 130x1003x64-flat (dh = 0 in exact arithmetic: the rows of E are equal and a dlogits row sums to zero)
    "grpo": 0.47,       # dlogp of B = 8, C = 700 with old_logp, beta = 0.04
}
# 2 x the twin: the factor 2 is for what the twin does not model — the hardware's exp2 / log2 (an ulp each, not the CPU's), fp32
# accumulation order inside the MFMA on the random sets, -ffast-math contraction.
MARGIN = {k_: 2 * v_ for k_, v_ in TWIN_WORST.items()}

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIO_FILE = os.path.join(os.environ.get("BRA_TEST_EVIDENCE_DIR") or os.path.join(ROOT, "test_evidence"), "loss_path_rowwise_ratios.json")


def _bf(x):
    return x.to(BF).to(F64)


def _ratio(err, E):
    """max err / E; an error where the bound is zero is infinite"""
    r = torch.where(E > 0, err / E.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return r.max().item() if r.numel() else 0.0


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


# ----------------------------------------------------------------------------- dispatch mirror
def _pick_variant(M, N, K, forced=-1, K2=0):
    if forced >= 0:
        return 6 if forced >= 6 else forced
    if K % 64 == 0 and K2 % 64 == 0:
        t = -(-M // 256) * -(-N // 256)
        rounds = -(-t // 256)
        if t >= 140 and (t <= 256 or 100 * t >= 60 * rounds * 256):
            return 6
        if -(-M // 256) * -(-N // 128) >= 128 or -(-M // 128) * -(-N // 128) >= 128:
            return 5
    return 0


def _glds_rows(M, N, forced=-1):
    if forced in (9, 10):
        return 192 if forced == 9 else 128
    if forced >= 0:
        return 256
    best, best_cost = 256, 1e30
    for bm, eff in ((256, 1.0), (192, 0.95), (128, 0.86)):
        t = -(-M // bm) * -(-N // 128)
        cost = -(-t // 256) * bm / eff
        if cost < best_cost * 0.97:
            best, best_cost = bm, cost
    return best


def _kernel(M, N, K, forced=-1):
    """the kernel bra_lmhead_lse_partials / bra_lmhead_dlogits launch for [M, K] x [N, K]^T; forced = the bra_gemm_set_variant argument"""
    v = _pick_variant(M, N, K, 5 if forced in (9, 10) else forced)
    if K % 64 == 0 and v == 6:
        return "ring"
    if K % 64 == 0 and v >= 4:
        return f"glds{_glds_rows(M, N, forced)}"
    return "nt256" if v in (2, 3) else "nt128"


# bra_gemm_bf16_nt (tests/test_gemm_family_rowwise.py): the same functions plus the second operand pair, the skinny kernel, pick_w4 and
# ring_split_rows.  No knob: the product library's choice is a pure function of (M, N, K, K2).
W4_TILES = {1: (160, 256), 2: (128, 256), 3: (160, 128), 4: (128, 128)}


def _pick_w4(M, N, K, K2=0):
    """pick_w4: the four-wave configuration (1..4) when it is the argmin of the launch-time model, else 0"""
    if K % 64 or K2 % 64 or M < 128 or N < 128 or K + K2 < 256:
        return 0
    if -(-M // 256) * -(-N // 256) > 256:
        return 0
    cands = ((256, 256, 5.9, 0), (256, 128, 4.27, 0), (192, 128, 4.56, 0), (128, 128, 3.75, 0),
             (160, 256, 4.5, 1), (128, 256, 4.5, 2), (160, 128, 4.5, 3), (128, 128, 4.5, 4))
    kk = 2.0e-6 * float(K + K2)
    best, best_t = 0, 1e30
    for bm, bn, rate, w4 in cands:
        tiles = -(-M // bm) * -(-N // bn)
        t = float(-(-tiles // 256)) * (kk * bm * bn / rate + 3.5)
        if t < best_t:
            best_t, best = t, w4
    return best


def _ring_split_rows(M, N, K, K2=0):
    """ring_split_rows: rows of the ring part when the last round of 256 x 256 tiles is less than half full, else 0"""
    if K % 64 or K2 % 64 or _pick_variant(M, N, K, K2=K2) != 6 or _pick_w4(M, N, K, K2):
        return 0
    tm, tn = -(-M // 256), -(-N // 256)
    t = tm * tn
    R = t // 256
    rem = t - R * 256
    if R < 1 or rem == 0 or 2 * rem >= 256:
        return 0
    rm = (R * 256) // tn
    if rm <= 0 or rm >= tm:
        return 0
    halves = -(-(M - rm * 256) // 256) * -(-N // 128)
    if halves < 32 or N * (K + K2) < 6 * 1024 * 1024:
        return 0
    return rm * 256 if R + 0.55 * -(-halves // 256) < (R + 1) - 0.15 else 0


def _route_bf16(M, N, K, K2=0):
    """the kernel(s) bra_gemm_bf16_nt launches in the product library: skinny | split (ring + LDS-DMA 256 rows) | w4-1..4 | ring |
    glds256 / 192 / 128 | nt128 (K % 64 != 0: its BK = 32 instance)"""
    if M <= 16:
        return "skinny"
    if _ring_split_rows(M, N, K, K2) > 0:
        return "split"
    if K % 64 == 0 and K2 % 64 == 0:
        w4 = _pick_w4(M, N, K, K2)
        if w4:
            return f"w4-{w4}"
        v = _pick_variant(M, N, K, K2=K2)
        if v == 6:
            return "ring"
        if v >= 4:
            return f"glds{_glds_rows(M, N)}"
    return "nt128"


FAMILY = {"nt128": "register-staged", "nt256": "register-staged", "ring": "ring", "glds256": "LDS-DMA", "glds192": "LDS-DMA", "glds128": "LDS-DMA"}
PINNED = {0: "nt128", 2: "nt256", 5: "glds256", 9: "glds192", 10: "glds128", 6: "ring"}
PINNED_SHAPES = [(330, 300, 64), (257, 520, 128)]

# ----------------------------------------------------------------------------- cases
EXACT = ("ints", "sparse", "sweep", "peaked", "flat")
# name: (M, V, K, values, option)   option: None | "strided" (h = a column slice of a wider tensor) | "notgt" (every fifth tgt = -1)
CASES = {}
for _M, _V, _K, _vals, _opt in [
    (330, 300, 64, "sweep", None), (330, 301, 64, "sweep", None), (130, 128, 64, "sweep", None), (70, 64, 64, "sweep", None),
    (70, 65, 64, "sweep", None), (330, 300, 96, "sweep", None), (330, 128, 128, "sweep", "strided"),
    (70, 300, 64, "ints", None), (130, 1000, 64, "ints", "notgt"), (17, 1003, 64, "ints", None), (1, 300, 64, "ints", None),
    (130, 1000, 128, "ints", None), (70, 300, 96, "ints", "strided"), (1, 64, 128, "ints", None),
    (70, 300, 64, "sparse", None), (130, 1000, 128, "sparse", None), (17, 128, 96, "sparse", None), (330, 1003, 96, "sparse", None),
    (130, 1000, 64, "peaked", None), (70, 300, 64, "peaked", None), (17, 65, 64, "peaked", None), (70, 301, 64, "peaked", None),
    (70, 300, 64, "flat", None), (17, 65, 64, "flat", None), (130, 1003, 64, "flat", None),
    (70, 300, 64, "rand", None), (130, 1000, 128, "rand", "notgt"), (330, 1003, 96, "rand", None), (1, 64, 64, "rand", None),
    (330, 128, 96, "rand", "strided"), (17, 1000, 96, "rand", None),
    (70, 300, 64, "big", None), (130, 301, 64, "big", None), (130, 1000, 128, "big", "strided"), (17, 65, 128, "big", None),
]:
    CASES[f"{_M}x{_V}x{_K}-{_vals}" + (f"-{_opt}" if _opt else "")] = (_M, _V, _K, _vals, _opt)
# the shapes at which the product library leaves the register-staged kernel (device only; see the module docstring)
BIG_CASES = {"300x17700x64-ring": (300, 17700, 64, "ring"), "256x16400x64-glds256": (256, 16400, 64, "glds256"),
             "384x11100x64-glds192": (384, 11100, 64, "glds192"), "256x8200x64-glds128": (256, 8200, 64, "glds128")}


def placed_targets(V):
    """the columns where the epilogues change behaviour: 64-column chunk edges, 16-column fragment edges, the first / last 4-group, the
    last multiple of 4 below V, V - 2, V - 1"""
    return sorted({t for t in (0, 3, 4, 15, 16, 63, 64, 127, 128, (V - 1) // 4 * 4, V - 2, V - 1) if 0 <= t < V})


def edge_columns(V):
    """placed_targets plus the chunk / tile edges of the last 256-column tile (the large-V cases)"""
    last = (V - 1) // 256 * 256
    cols = set(placed_targets(V)) | {last - 1, last, last + 63, last + 64, last + 127, last + 128, (V - 1) // 64 * 64 - 1, (V - 1) // 64 * 64}
    return sorted(c for c in cols if 0 <= c < V)


def _randint(g, shape, a):
    return torch.randint(-a, a + 1, shape, generator=g).float()


@functools.lru_cache(maxsize=None)
def _operands(M, V, K, vals, dom_cols=None):
    """-> (h [M, K], e [V, K]) bf16 on the CPU, tgt [M] int32, coef [M] fp32.  Exact sets: K max|h| max|e| <= 256."""
    g = torch.Generator().manual_seed(1000 * M + 7 * V + K)
    T = placed_targets(V)
    tgt = torch.tensor([T[i % len(T)] for i in range(M)], dtype=torch.int32)
    if vals == "ints":
        h, e = _randint(g, (M, K), 2 if K <= 64 else 1), _randint(g, (V, K), 2)
    elif vals == "sparse":
        h = _randint(g, (M, K), 1) * (torch.rand(M, K, generator=g) < 0.4)
        e = _randint(g, (V, K), 1) * (torch.rand(V, K, generator=g) < 0.4)
    elif vals == "sweep":
        # +-1 codes on the first 64 coordinates (the others stay zero): x[i, dom(i)] = 128, the rest 2 (code . code) ~ N(0, 16^2)
        code = torch.randint(0, 2, (V, 64), generator=g).float() * 2 - 1
        dom = torch.tensor(dom_cols, dtype=torch.long)[torch.arange(M) % len(dom_cols)] if dom_cols else torch.arange(M) % V
        e, h = torch.zeros(V, K), torch.zeros(M, K)
        e[:, :64], h[:, :64] = code, 2 * code[dom]
    elif vals == "peaked":
        # the targets are the dominant columns: five coordinates per placed target (x_t = 5 * 2 * 2 = 20), four noise coordinates in {-1, 0, 1} that the target columns
        # do not have: every other logit is within [-4, 4], p_t >= 1 - V e^-16
        assert K == 64 and len(T) <= 12
        e, h = torch.zeros(V, K), torch.zeros(M, K)
        e[:, 60:], h[:, 60:] = _randint(g, (V, 4), 1), _randint(g, (M, 4), 1)
        for a, t in enumerate(T):
            e[t, 5 * a:5 * a + 5], e[t, 60:] = 2, 0
        for i in range(M):
            a = i % len(T)
            h[i, 5 * a:5 * a + 5] = 2
    elif vals == "flat":
        e, h = torch.zeros(V, K), torch.zeros(M, K)
        e[:, :2], h[:, 0], h[:, 1] = 1, 2, 1
    else:
        s = 0.5 if vals == "rand" else (30 / (3.5 * math.sqrt(K))) ** 0.5
        h, e = torch.randn(M, K, generator=g) * s, torch.randn(V, K, generator=g) * s
    coef = torch.randn(M, generator=g)
    coef[1::7] = 0                                         # masked tokens
    coef[::5] = -coef[::5].abs() - 0.5                     # and negative coefficients for certain
    if M == 1:
        coef[0] = -1.5
    return h.to(BF), e.to(BF), tgt, coef.to(F32)


# ----------------------------------------------------------------------------- float64 reference, bounds, twin
def _lse32(xb):
    """float32 restatement of the EPI_LSE epilogue and lse_merge_kernel on logits xb [M, V]: per 64-column chunk the maximum and the
    sum of exp(x - max) in the lanes' order (lane fq of a row holds columns 16 ni + 4 fq + r: 16 sequential additions, then the two
    cross-lane steps), the merge over chunks (lane = chunk, then the butterfly), exp(a) = exp2(a log2 e), log(s) = log2(s) ln 2"""
    M, V = xb.shape
    nch = -(-V // 64)
    x = torch.full((M, nch * 64), -math.inf, dtype=F32, device=xb.device)
    x[:, :V] = xb.to(F32)
    x = x.view(M, nch, 4, 4, 4)                                    # [chunk][ni][fq][r]
    cm = x.amax((2, 3, 4))
    ex = torch.exp2((x - cm[:, :, None, None, None]) * LOG2E).permute(0, 1, 3, 2, 4).reshape(M, nch, 4, 16)
    s = ex[..., 0].clone()
    for i in range(1, 16):
        s = s + ex[..., i]
    s = s + s[..., [1, 0, 3, 2]]
    s = s + s[..., [2, 3, 0, 1]]
    m = cm.amax(1)
    t = s[..., 0] * torch.exp2((cm - m[:, None]) * LOG2E)
    lanes = torch.zeros(M, 64, dtype=F32, device=xb.device)
    for c0 in range(0, nch, 64):
        blk = t[:, c0:c0 + 64]
        lanes[:, :blk.shape[1]] = lanes[:, :blk.shape[1]] + blk
    for half in (32, 16, 8, 4, 2, 1):
        lanes = lanes[:, :half] + lanes[:, half:2 * half]
    return m + torch.log2(lanes[:, 0]) * LN2


def _exp32(a):
    return torch.exp2(a.to(F32) * LOG2E)


def _lmhead_ref(h, e, tgt, coef, exact):
    """float64 reference and bound vectors for one case, on h's device.  -> dict"""
    x = h.to(F64) @ e.to(F64).T
    M, V = x.shape
    lse = torch.logsumexp(x, -1)
    m = x.max(-1).values
    p = torch.exp(x - lse[:, None])
    has = tgt >= 0
    xt = torch.where(has, x.gather(1, tgt.clamp(min=0).long()[:, None])[:, 0], torch.zeros_like(lse))
    logp = xt - lse
    spx = (p * x.abs()).sum(-1)
    f_lse = U32 * (2 * (p * (m[:, None] - x)).sum(-1) + 8 + 3 * (lse - m).abs() + lse.abs())
    f_logp = f_lse + U32 * logp.abs()
    rb = 0.0 if exact else U                                        # the logits' own bf16 rounding: none on the exact sets
    onehot = torch.zeros_like(x)
    onehot[has, tgt[has].long()] = 1.0
    c = coef.to(F64)[:, None]
    dl = c * (onehot - p)
    f_p = U32 * (2 + 3 * (x - lse[:, None]).abs())
    r = {"x": x, "lse": lse, "logp": logp, "p": p, "dl": dl, "onehot": onehot,
         "E_lse": rb * spx + f_lse, "E_logp": rb * (xt.abs() + spx) + f_logp, "f_lse": f_lse}

    def dl_bound(lse_err):
        """element bound of dlogits when the lse it is fed is within lse_err [M] of the row's"""
        return U * dl.abs() + c.abs() * p * (f_p + lse_err[:, None] + rb * (x.abs() + spx[:, None])) + TINY * (1 + c.abs())

    r["dl_bound"] = dl_bound
    r["dh"] = dl @ e.to(F64)
    r["dh_bound"] = lambda b: U * r["dh"].abs() + (b + V * U32 * dl.abs()) @ e.to(F64).abs()
    return r


def _lmhead_twin(h, e, tgt, coef, ref):
    """the rounding twin: (lse, logp, dlogits, dh) from the bf16-rounded float64 logits through the float32 restatement"""
    xb = _bf(ref["x"])
    lse = _lse32(xb)
    has = tgt >= 0
    xt = torch.where(has, xb.gather(1, tgt.clamp(min=0).long()[:, None])[:, 0], torch.zeros_like(xb[:, 0])).to(F32)
    logp = xt - lse
    p32 = _exp32(xb.to(F32) - lse[:, None])
    dl = (coef[:, None] * (ref["onehot"].to(F32) - p32)).to(BF)
    dh = (dl.to(F64) @ e.to(F64)).to(F32).to(BF)
    return lse, logp, dl, dh


def _compare(ref, exact, lse, logp, dl_own, dl_fed, dh, coef):
    """worst ratios of the kernels' (or the twin's) results; dl_own: dlogits fed the same run's lse, dl_fed: fed fp32(float64 lse)"""
    sfx = "32" if exact else ""                                     # exact sets: the fp32 term alone, with its own margin
    out = {"lse" + sfx: _ratio((lse.to(F64) - ref["lse"]).abs(), ref["E_lse"]),
           "logp" + sfx: _ratio((logp.to(F64) - ref["logp"]).abs(), ref["E_logp"])}
    key = "dl_elem" if exact else "dl_row"
    for name, got, lse_err in (("own", dl_own, ref["E_lse"]), ("fed", dl_fed, U32 * ref["lse"].abs())):
        if got is None:
            continue
        b = ref["dl_bound"](lse_err)
        err = (got.to(F64) - ref["dl"]).abs()
        out[f"{key}_{name}"] = _ratio(err, b) if exact else _ratio(err.norm(dim=-1), b.norm(dim=-1))
        assert (got[coef == 0] == 0).all(), "a row with coef = 0 must be exactly zero"
    if dh is not None:
        b = ref["dh_bound"](ref["dl_bound"](ref["E_lse"]))
        out["dh"] = _ratio((dh.to(F64) - ref["dh"]).norm(dim=-1), b.norm(dim=-1))
    return out


def _assert_ratios(name, ratios, dev):
    print(f"\n[loss-path] {name}: " + " ".join(f"{k_} {v_:.3f}" for k_, v_ in ratios.items()))
    _record(name, ratios, dev)
    for k_, v_ in ratios.items():
        base = k_.rsplit("_", 1)[0] if k_.endswith(("_own", "_fed")) else k_
        assert v_ <= MARGIN[base], (name, k_, v_, MARGIN[base])


def _dh_kernels(dl, e):
    """dh = ops.gemm_nt(dlogits, E^T) as modeling._LogProbFn.backward forms it (see the module docstring for V % 32 != 0)"""
    M, V = dl.shape
    if V % 32 == 0:
        ET = ops.transpose2d(e, pad_to=256)                          # [K, 256 n]: the ET[:, :V] slice of a wider image
        assert ET.shape[1] != V or V % 256 == 0
        return ops.gemm_nt(dl, ET[:, :V])
    with pytest.raises(_lib.KernelError) as ei:                      # the contraction length must be a multiple of 32
        ops.gemm_nt(dl, ops.transpose2d(e)[:, :V])
    assert ei.value.status == _lib.BRA_ERR_ARG
    Vp = -(-V // 32) * 32
    wide = torch.zeros(M, Vp, dtype=BF, device=dl.device)
    wide[:, :V] = dl
    return ops.gemm_nt(wide, ops.transpose2d(e, pad_to=32))


def _run_case(name, dev, M, V, K, vals, opt, dom_cols=None, with_dh=True):
    exact = vals in EXACT
    h0, e0, tgt0, coef0 = _operands(M, V, K, vals, dom_cols)
    tgt0 = tgt0.clone()
    if opt == "notgt":
        tgt0[::5] = -1
    h, e, tgt, coef = h0.to(dev), e0.to(dev), tgt0.to(dev), coef0.to(dev)
    if opt == "strided":
        wide = torch.full((M, K + 72), float("nan"), dtype=BF, device=dev)
        wide[:, 8:8 + K] = h
        h = wide[:, 8:8 + K]
        assert h.stride(0) != K
    ref = _lmhead_ref(h, e, tgt, coef, exact)
    if exact:
        assert torch.equal(_bf(ref["x"]), ref["x"]) and ref["x"].abs().max() <= 256      # every logit is a bf16 number
    if vals == "peaked":
        assert (ref["p"].gather(1, tgt.long()[:, None]) >= 1 - 1e-4).all()
    if vals == "flat":
        assert torch.allclose(ref["lse"], ref["x"][:, 0] + math.log(V), rtol=0, atol=1e-12)
    logp, lse = ops.lmhead_logprob(h, e, tgt)
    if opt == "notgt":
        assert torch.equal(logp[tgt < 0], 0 - lse[tgt < 0])
    dl_own = dl_fed = dh = None
    if V % 4 == 0:
        dl_own = ops.lmhead_dlogits(h, e, tgt, lse, coef)
        dl_fed = ops.lmhead_dlogits(h, e, tgt, ref["lse"].to(F32), coef)
        if with_dh:
            dh = _dh_kernels(dl_own, e)
    ratios = _compare(ref, exact, lse, logp, dl_own, dl_fed, dh, coef)
    _assert_ratios(name, ratios, dev)
    return ratios


# ----------------------------------------------------------------------------- 1 + 2: lm_head log-prob, dlogits, dh
@pytest.mark.parametrize("name", list(CASES))
def test_lmhead_rowwise(backend, name):
    """lse and logp per row, dlogits per element (exact sets) / per row (random sets) fed its own and the reference's lse, dh per row"""
    M, V, K, vals, opt = CASES[name]
    assert _kernel(M, V, K) == "nt128"
    _run_case(name, backend, M, V, K, vals, opt)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BIG_CASES))
def test_lmhead_rowwise_product_dispatch(hip_device, name):
    """the ring and the LDS-DMA kernel as the product library dispatches them: exact logits, every row's dominant logit on an edge
    column of the first / last tiles, targets on the same list one step on"""
    M, V, K, kern = BIG_CASES[name]
    assert _kernel(M, V, K) == kern
    _run_case(name, hip_device, M, V, K, "sweep", None, dom_cols=tuple(edge_columns(V)), with_dh=False)


@pytest.mark.parametrize("variant", list(PINNED))
def test_lmhead_rowwise_pinned_variants(debug_backend, variant):
    """both epilogue copies (gemm_epilogue; gemm_epilogue_w at MI = 2, 3, 4 and in the ring kernel) under the row-wise bound"""
    lib = _lib.get_lib()
    try:
        lib.call("bra_gemm_set_variant", variant)
        for (M, V, K) in PINNED_SHAPES:
            assert _kernel(M, V, K, variant) == PINNED[variant]
            for vals in ("sweep", "rand") if M >= V else ("ints", "big"):
                _run_case(f"v{variant}-{M}x{V}x{K}-{vals}", debug_backend, M, V, K, vals, None, with_dh=False)
    finally:
        lib.call("bra_gemm_set_variant", -1)


def test_dlogits_refuses_ragged_rows(backend):
    """V % 4 != 0: ops.lmhead_dlogits raises; the entry point returns BRA_ERR_ARG for the pitch before any launch (buffer untouched)"""
    M, V, K = 17, 301, 64
    h0, e0, tgt0, coef0 = _operands(M, V, K, "ints")
    h, e, tgt, coef = h0.to(backend), e0.to(backend), tgt0.to(backend), coef0.to(backend)
    _, lse = ops.lmhead_logprob(h, e, tgt)
    with pytest.raises(_lib.KernelError) as ei:
        ops.lmhead_dlogits(h, e, tgt, lse, coef)
    assert ei.value.status == _lib.BRA_ERR_ARG
    out = torch.full((M, V), 3.0, dtype=BF, device=backend)
    with pytest.raises(_lib.KernelError) as ei:
        _lib.get_lib().call("bra_lmhead_dlogits", h, K, e, K, M, V, K, tgt, lse, coef, out, V, _lib.current_stream(h))
    assert ei.value.status == _lib.BRA_ERR_ARG and (out.float() == 3.0).all()


# ----------------------------------------------------------------------------- 3: dispatch
def test_dispatch_mirror_and_coverage():
    """every case takes the kernel written next to it; the emulator leg covers every pinned variant, the device leg adds the shapes
    at which the product library takes the ring and the LDS-DMA kernel (at its three tile heights): all three GEMM kernels"""
    assert _kernel(300, 17700, 64) == "ring" and _kernel(256, 16400, 64) == "glds256"
    assert _kernel(256, 8200, 64) == "glds128" and _kernel(384, 11100, 64) == "glds192"
    assert _kernel(256, 8064, 64) == "nt128"                          # 2 x 64 = 128 tiles of 128 x 128 are the threshold: 126 here
    assert _kernel(300, 17664, 64) != "ring" and _kernel(300, 17665, 64) == "ring"         # 138 / 140 ring tiles
    assert _kernel(300, 17700, 96) == "nt128"                         # K % 64 != 0: the BK = 32 instance of the register-staged kernel
    # the step's own lm_head: (B C, 151 936, 2048) with B C in the thousands
    assert _kernel(2048, 151936, 2048) == "ring"
    product = {FAMILY[_kernel(M, V, K)] for (M, V, K, _, _) in CASES.values()}
    assert product == {"register-staged"}
    product |= {FAMILY[_kernel(M, V, K)] for (M, V, K, _) in BIG_CASES.values()}
    assert product == {"register-staged", "ring", "LDS-DMA"}
    pinned = {_kernel(M, V, K, v) for v in PINNED for (M, V, K) in PINNED_SHAPES}
    assert pinned == {"nt128", "nt256", "glds256", "glds192", "glds128", "ring"}
    for v, k_ in PINNED.items():
        for (M, V, K) in PINNED_SHAPES:
            assert _kernel(M, V, K, v) == k_


# ----------------------------------------------------------------------------- the twin
TWIN_CASES = list(CASES) + [f"pinned-{M}x{V}x{K}-{vals}" for (M, V, K) in PINNED_SHAPES for vals in (("sweep", "rand") if M >= V else ("ints", "big"))]


def _twin_worst():
    worst, where = dict.fromkeys(("lse32", "logp32", "lse", "logp", "dl_elem", "dl_row", "dh"), 0.0), {}
    for name in TWIN_CASES:
        if name in CASES:
            M, V, K, vals, opt = CASES[name]
        else:
            M, V, K = (int(t) for t in name.split("-")[1].split("x"))
            vals, opt = name.split("-")[2], None
        h, e, tgt, coef = _operands(M, V, K, vals)
        if opt == "notgt":
            tgt = tgt.clone()
            tgt[::5] = -1
        exact = vals in EXACT
        ref = _lmhead_ref(h, e, tgt, coef, exact)
        lse, logp, dl, dh = _lmhead_twin(h, e, tgt, coef, ref)
        got = _compare(ref, exact, lse, logp, dl, None, dh, coef)
        for k_, v_ in got.items():
            k_ = k_.replace("_own", "")
            if v_ > worst[k_]:
                worst[k_], where[k_] = v_, name
    return worst, where


def test_twin_ratio_is_the_recorded_one():
    """MARGIN's origin, reproducible without a GPU and without project code"""
    worst, where = _twin_worst()
    gw, gwhere = _grpo_twin_worst()
    worst["grpo"], where["grpo"] = gw, gwhere
    print(f"\n[loss-path] twin worst ratios {worst} at {where}")
    for k_ in TWIN_WORST:
        # (to the two digits written; the fp32-level ones depend on the last bit of the host's exp2 / log2: two hundredths there)
        tol = 0.02 if k_ in ("lse32", "logp32", "grpo") else 0.01
        assert math.isfinite(worst[k_]) and abs(worst[k_] - TWIN_WORST[k_]) <= tol, (k_, worst[k_], where[k_])
        assert MARGIN[k_] == 2 * TWIN_WORST[k_]


# ----------------------------------------------------------------------------- 4: grpo_loss
EPS_LO, EPS_HI = 0.2, 0.3
# (B, C, old_logp given, beta)
GRPO_CASES = [(1, 1, False, 0.04), (1, 700, True, 0.04), (4, 255, True, 0.0), (4, 256, False, 0.04), (4, 257, True, 0.04),
              (8, 700, True, 0.04), (8, 700, False, 0.0), (8, 257, True, 0.0), (4, 1, True, 0.04), (8, 255, False, 0.04)]


@functools.lru_cache(maxsize=None)
def _grpo_inputs(B, C, use_old):
    """fp32 inputs on the CPU.  Ratios exp(lp - old) are placed: the two clamp edges 1 - eps_lo and 1 + eps_hi, each 16 fp32 ulp inside and
    16 ulp outside — exactly ON an edge is not reachable portably (libm's expf on the emulator, exp2(a log2 e) on the device and the
    float64 reference round differently, and the kernel's edge is the fp32 number 1.f - eps) — then far inside, far outside on both
    sides, and exactly 1 (old = lp: the tie l1 == l2).  Advantages: exact 0 (a zero-variance group), both signs, one large."""
    g = torch.Generator().manual_seed(100 * B + C)
    lp = -torch.rand(B, C, generator=g) * 3
    ref = lp + 0.2 * torch.randn(B, C, generator=g)
    adv = torch.tensor([0.0, 1.3, -0.7, 50.0, -2.5, 0.4, -50.0, 1e-3])[:B].clone()
    if B == 1:
        adv = torch.tensor([[-0.7, 1.3, 0.0, 50.0][C % 4]])
    lo, hi = 1 - float(torch.tensor(EPS_LO, dtype=F32)), 1 + float(torch.tensor(EPS_HI, dtype=F32))
    d8 = 16 * 2.0 ** -23
    logr = [math.log(lo * (1 + d8)), math.log(lo * (1 - d8)), math.log(hi * (1 - d8)), math.log(hi * (1 + d8)),
            0.05, -0.1, math.log(0.5), math.log(1.9), 0.0, 0.2, -0.15, 0.0]
    old = None
    if use_old:
        pat = torch.tensor(logr, dtype=F64)[(torch.arange(B * C) * 5 % len(logr)).view(B, C)]
        old = (lp.to(F64) - pat).to(F32)
        old[pat == 0] = lp[pat == 0]
    # masks as eos_mask makes them: a live prefix of length 1 .. C, one row fully live
    mask = torch.zeros(B, C, dtype=torch.int32)
    for b in range(B):
        n = C if b == B - 1 else 1 + (b * (C - 1)) // max(B - 1, 1)
        mask[b, :n] = 1
    return lp, old, ref, adv, mask


def _grpo_ref(lp, old, ref, adv, mask, beta):
    """float64: oracle/grpo_math.grpo_loss + autograd, the kernel's fp32 clamp edges handed over as the epsilons.  -> dict"""
    lo, hi = float(torch.tensor(1.0, dtype=F32) - torch.tensor(EPS_LO, dtype=F32)), float(torch.tensor(1.0, dtype=F32) + torch.tensor(EPS_HI, dtype=F32))
    lpt = lp.to(F64).requires_grad_(True)
    o = old.to(F64) if old is not None else None
    m = mask.to(F64)
    loss, kl, clip = grpo_math.grpo_loss(lpt, o, ref.to(F64), adv.to(F64), m, 1 - lo, hi - 1, beta)
    loss.backward()
    B, C = lp.shape
    with torch.no_grad():
        d = lpt.detach() - (o if o is not None else lpt.detach())
        c1 = torch.exp(d)
        A = adv.to(F64)[:, None].abs()
        ms = m.sum(1, keepdim=True)
        inside = (c1 >= lo) & (c1 <= hi)
        # -min(l1, l2) follows l1 = c1 A (gradient -A c1) inside the clamp, below it for A > 0 and above it for A < 0; elsewhere it is flat
        unclipped = inside | ((c1 < lo) & (adv[:, None] > 0)) | ((c1 > hi) & (adv[:, None] < 0))
        dl = ref.to(F64) - lpt.detach()
        e = torch.exp(dl)
        # fp32 roundoff on the policy term |A| c1 — the exponential's ulp (2 u), its argument (the subtraction u |d|, the product with
        # log2 e and the constant 1.5 u |d|), the product with A, the sum with the k3 term, the division: (5 + 3 |d|) u — and on the k3
        # term beta (1 - e): the error of e is absolute, u e (2 + 3 |dl|), whatever 1 - e cancels to, then 1 - e, the product with
        # beta, the sum and the division round once each.  The library is built with -ffast-math: a division may be a reciprocal (an
        # ulp, 2 u) and a product, 3 u instead of one — hence 7 and 6
        E = U32 * (A * c1 * unclipped * (7 + 3 * d.abs()) + beta * (e * (2 + 3 * dl.abs()) + 6 * (1 - e).abs())) * m / (ms * B)
        ptl = -torch.min(c1 * adv.to(F64)[:, None], c1.clamp(lo, hi) * adv.to(F64)[:, None])
        klt = (e - dl - 1) if beta > 0 else torch.zeros_like(e)
        # out3: per element the arithmetic above (<= 8 + 3 |d| + 3 |dl| roundings), then a sum of ceil(C / 256) sequential additions per
        # thread, six butterfly steps, four wave partials, the division and the mean over B: worst case, so ratio <= 1 without a margin
        nadd = -(-C // 256) + 6 + 4 + 3 + B
        per = (A * c1 * (8 + 3 * d.abs()) + beta * (e * (8 + 3 * dl.abs()) + dl.abs() + 1)) + nadd * (ptl + beta * klt).abs()
        E_loss = U32 * ((per * m).sum(1) / ms[:, 0]).mean().item() + U32 * abs(loss.item())
        per_kl = e * (8 + 3 * dl.abs()) + dl.abs() + 1 + nadd * klt.abs()
        E_kl = U32 * ((per_kl * m).sum(1) / ms[:, 0]).mean().item()
    return {"loss": loss.item(), "kl": kl.item() if kl is not None else 0.0, "clip": clip.item(), "dlogp": lpt.grad, "E": E,
            "E_loss": E_loss, "E_kl": E_kl}


def _grpo_twin(lp, old, ref, adv, mask, beta):
    """float32 torch restatement of grpo_loss_kernel's dlogp"""
    one = torch.tensor(1.0, dtype=F32)
    lo, hi = one - torch.tensor(EPS_LO, dtype=F32), one + torch.tensor(EPS_HI, dtype=F32)
    B, C = lp.shape
    A = adv[:, None]
    c1 = _exp32(lp - (old if old is not None else lp))
    c2 = torch.minimum(torch.maximum(c1, lo), hi)
    l1, l2 = c1 * A, c2 * A
    g1 = -A * c1
    g2 = torch.where((c1 >= lo) & (c1 <= hi), g1, torch.zeros_like(g1))
    gg = torch.where(l1 < l2, g1, torch.where(l1 > l2, g2, 0.5 * (g1 + g2)))
    if beta:
        gg = gg + torch.tensor(beta, dtype=F32) * (1 - _exp32(ref - lp))
    mk = mask.to(F32)
    ms = mk.sum(1, keepdim=True)
    return gg * mk / (ms * B)


def _grpo_twin_worst():
    worst, where = 0.0, None
    for (B, C, use_old, beta) in GRPO_CASES:
        lp, old, ref, adv, mask = _grpo_inputs(B, C, use_old)
        r = _grpo_ref(lp, old, ref, adv, mask, beta)
        w = _ratio((_grpo_twin(lp, old, ref, adv, mask, beta).to(F64) - r["dlogp"]).abs(), r["E"])
        if w > worst:
            worst, where = w, (B, C, use_old, beta)
    return worst, where


@pytest.mark.parametrize("B,C,use_old,beta", GRPO_CASES)
def test_grpo_loss_elementwise(backend, B, C, use_old, beta):
    """dlogp element by element (masked entries exactly 0), out3 within worst-case fp32 bounds that grow with the summed magnitudes,
    need_grad=False leaves out3 unchanged; C up to 700: the `c += 256` loop runs three times"""
    dev = backend
    lp, old, ref, adv, mask = _grpo_inputs(B, C, use_old)
    r = _grpo_ref(lp, old, ref, adv, mask, beta)
    args = (lp.to(dev), old.to(dev) if old is not None else None, ref.to(dev) if beta else None, adv.to(dev), mask.to(dev))
    out3, dlogp = ops.grpo_loss(*args, EPS_LO, EPS_HI, beta)
    out3b, none = ops.grpo_loss(*args, EPS_LO, EPS_HI, beta, need_grad=False)
    assert none is None and torch.equal(out3.cpu(), out3b.cpu())
    dlogp, out3 = dlogp.cpu(), out3.cpu().to(F64)
    assert (dlogp[mask == 0] == 0).all()
    ratios = {"grpo": _ratio((dlogp.to(F64) - r["dlogp"]).abs(), r["E"]),
              "loss": abs(out3[0].item() - r["loss"]) / r["E_loss"],
              "kl": abs(out3[1].item() - r["kl"]) / r["E_kl"] if beta else 0.0}
    name = f"grpo-B{B}-C{C}-{'old' if use_old else 'noold'}-beta{beta}"
    print(f"\n[loss-path] {name}: " + " ".join(f"{k_} {v_:.3f}" for k_, v_ in ratios.items()))
    _record(name, ratios, dev)
    assert ratios["grpo"] <= MARGIN["grpo"], ratios
    assert ratios["loss"] <= 1.0 and ratios["kl"] <= 1.0, ratios
    if not beta:
        assert out3[1].item() == 0.0
    # clip_ratio: whole-number counts (exact in fp32) and one division
    assert abs(out3[2].item() - r["clip"]) <= 4 * U32 * max(r["clip"], 1e-30) + 0.0
    if not use_old:
        # the tie branch everywhere: c1 == 1, nothing clipped, gradient -A (+ the k3 term)
        assert out3[2].item() == 0.0


# ----------------------------------------------------------------------------- 4: group_advantage, eos_mask
@pytest.mark.parametrize("G", [2, 4, 8, 64])
@pytest.mark.parametrize("F", [1, 2, 5])
def test_group_advantage_vs_float64(backend, G, F):
    """adv, grp_mean, grp_std against oracle/grpo_math.group_advantages in float64, worst-case fp32 bounds (ratio <= 1); a group of identical
    rewards gives adv exactly 0 and std 0 (G is a power of two: the butterfly sum of G equal numbers and the division by G are exact)"""
    dev = backend
    ngrp = 5
    g = torch.Generator().manual_seed(10 * G + F)
    r = torch.randn(ngrp, G, F, generator=g)
    r[1] = (torch.arange(F, dtype=F32) * 0.25 + 0.5)[None, :]        # identical rewards: a zero-variance group
    r[2] = r[2, :1]
    r[2, G - 1] += 100.0                                              # a single outlier
    r[3] = r[3] * 1e-3 + 2.0                                          # a small spread on a large mean: r - mean cancels
    r = r.view(ngrp * G, F).contiguous()
    adv, gm, gs = ops.group_advantage(r.to(dev), G)
    adv, gm, gs = adv.cpu().to(F64), gm.cpu().to(F64), gs.cpu().to(F64)
    want, mean, std = grpo_math.group_advantages(r.to(F64), G)
    R = r.to(F64).abs().sum(1).view(ngrp, G).max(1).values           # max_i sum_f |r_if| of the group
    # (a division may be a reciprocal and a product under -ffast-math: 3 u; the hardware square root: an ulp, 2 u)
    dd = U32 * (F + 11) * R                                           # r_i (F additions), the mean (6 butterfly steps, the division), r - mean
    sd = std.view(ngrp, G)[:, 0]
    dsd = dd * math.sqrt(G / (G - 1)) + U32 * (math.log2(G) + 8) * sd   # | ||d + dd|| - ||d|| | <= ||dd||, then the squares, sum, division, sqrt
    dadv = (dd[:, None] + want.view(ngrp, G).abs() * (dsd[:, None] + U32 * sd[:, None])) / (sd[:, None] + 1e-4) + 5 * U32 * want.view(ngrp, G).abs()
    ratios = {"adv": _ratio((adv - want).abs().view(ngrp, G), dadv), "mean": _ratio((gm - mean.view(ngrp, G)[:, 0]).abs(), dd),
              "std": _ratio((gs - sd).abs(), dsd)}
    print(f"\n[loss-path] group_advantage G{G} F{F}: " + " ".join(f"{k_} {v_:.3f}" for k_, v_ in ratios.items()))
    _record(f"group_advantage-G{G}-F{F}", ratios, dev)
    assert max(ratios.values()) <= 1.0, ratios
    assert (adv.view(ngrp, G)[1] == 0).all() and gs[1].item() == 0.0 and sd[1].item() == 0.0


def test_group_advantage_refusals(backend):
    """G = 65 (one wave holds a group) and N % G != 0 are BRA_ERR_ARG, nothing written"""
    for N, G in ((130, 65), (10, 4)):
        r = torch.ones(N, 2, device=backend)
        adv = torch.full((N,), 7.0, device=backend)
        gm, gs = torch.full((N,), 7.0, device=backend), torch.full((N,), 7.0, device=backend)
        with pytest.raises(_lib.KernelError) as ei:
            _lib.get_lib().call("bra_group_advantage", r, N, 2, G, adv, gm, gs, _lib.current_stream(r))
        assert ei.value.status == _lib.BRA_ERR_ARG
        assert (adv == 7).all() and (gm == 7).all() and (gs == 7).all()
    with pytest.raises(_lib.KernelError):
        ops.group_advantage(torch.ones(130, 2, device=backend), 65)


@pytest.mark.parametrize("C", [1, 63, 64, 65, 200])
def test_eos_mask_exact(backend, C):
    """first EOS at 0, 63, 64, C - 1 or absent, two EOS in one row: exactly oracle/grpo_math.completion_mask, lengths = its row sums"""
    eos = 2
    firsts = sorted({f for f in (0, 63, 64, C - 1) if f < C})
    rows = []
    for f in firsts + [None]:
        row = torch.randint(3, 50, (C,), generator=torch.Generator().manual_seed(C + (f or 0)))
        if f is not None:
            row[f] = eos
        rows.append(row)
        if f is not None and f + 1 < C:                              # a second EOS later in the row changes nothing
            row2 = row.clone()
            row2[(f + 1 + C) // 2] = eos
            row2[C - 1] = eos
            rows.append(row2)
    ids = torch.stack(rows).to(torch.int32)
    mask, lengths = ops.eos_mask(ids.to(backend), eos)
    want = grpo_math.completion_mask(ids.long(), eos)
    assert torch.equal(mask.cpu(), want.to(torch.int32)) and torch.equal(lengths.cpu().long(), want.sum(1))


# ----------------------------------------------------------------------------- 5: the chain
def test_loss_chain_rowwise(backend):
    """lmhead_logprob -> grpo_loss -> lmhead_dlogits(coef = dlogp) -> gemm_nt(E^T), as grpo.py and modeling._LogProbFn compose them,
    against float64 autograd of loss(h), row by row on dL/dh; exact logits (M = B C = 4 x 65, V = 300, K = 64)"""
    dev = backend
    B, C, V, K, beta = 4, 65, 300, 64, 0.04
    M = B * C
    h0, e0, tgt0, _ = _operands(M, V, K, "sparse")
    h, e, tgt = h0.to(dev), e0.to(dev), tgt0.to(dev)
    g = torch.Generator().manual_seed(5)
    adv = torch.tensor([1.3, -0.7, 0.0, 2.5])
    mask = torch.zeros(B, C, dtype=torch.int32)
    for b, n in enumerate((1, 23, 64, 65)):
        mask[b, :n] = 1
    # float64: the whole expression loss(h)
    hd = h0.to(F64).requires_grad_(True)
    x = hd @ e0.to(F64).T
    lp64 = (x.gather(1, tgt0.long()[:, None])[:, 0] - torch.logsumexp(x, -1)).view(B, C)
    old = (lp64.detach() + 0.25 * torch.randn(B, C, generator=g).to(F64)).to(F32)
    refl = (lp64.detach() + 0.2 * torch.randn(B, C, generator=g).to(F64)).to(F32)
    lo, hi = float(torch.tensor(1.0, dtype=F32) - torch.tensor(EPS_LO, dtype=F32)), float(torch.tensor(1.0, dtype=F32) + torch.tensor(EPS_HI, dtype=F32))
    loss, _, _ = grpo_math.grpo_loss(lp64, old.to(F64), refl.to(F64), adv.to(F64), mask.to(F64), 1 - lo, hi - 1, beta)
    loss.backward()
    # the kernels
    logp, lse = ops.lmhead_logprob(h, e, tgt)
    out3, dlogp = ops.grpo_loss(logp.view(B, C), old.to(dev), refl.to(dev), adv.to(dev), mask.to(dev), EPS_LO, EPS_HI, beta)
    coef = dlogp.reshape(M).contiguous().float()
    dh = _dh_kernels(ops.lmhead_dlogits(h, e, tgt, lse, coef), e)
    # the bound: the lm_head bounds with coef = the float64 dL/dlogp, plus what an error of coef itself moves — the grpo element bound
    # and, through exp(lp - old) and exp(ref - lp), the error of the logp the loss kernel is fed (|d coef / d logp| <= |coef| + beta e / (ms B))
    lp_d = lp64.detach()
    r = _grpo_ref(lp_d.to(F32), old, refl, adv, mask, beta)                  # (E and E_loss of the grpo stage at these inputs)
    lpq = lp_d.clone().requires_grad_(True)
    grpo_math.grpo_loss(lpq, old.to(F64), refl.to(F64), adv.to(F64), mask.to(F64), 1 - lo, hi - 1, beta)[0].backward()
    coef64 = lpq.grad.reshape(M)
    ref = _lmhead_ref(h0, e0, tgt0, coef64, True)
    ms = mask.to(F64).sum(1, keepdim=True)
    dlogp_in = (MARGIN["logp32"] * ref["E_logp"] + U32 * lp_d.reshape(M).abs()).view(B, C)      # error of the kernels' logp (+ the fp32 copy)
    dcoef = (MARGIN["grpo"] * r["E"] + (coef64.view(B, C).abs() + beta * torch.exp(refl.to(F64) - lp_d) * mask / (ms * B)) * dlogp_in).reshape(M)
    # (dcoef carries its margins already: divided by MARGIN["dh"] here, multiplied back by the assertion)
    b_dl = ref["dl_bound"](ref["E_lse"]) + dcoef[:, None] * (ref["onehot"] - ref["p"]).abs() / MARGIN["dh"]
    E = ref["dh_bound"](b_dl)
    E_loss = r["E_loss"] + (coef64.view(B, C).abs() * dlogp_in).sum().item()               # first order: dL = sum coef dlogp
    ratios = {"dh": _ratio((dh.cpu().to(F64) - hd.grad).norm(dim=-1), E.norm(dim=-1)), "loss": abs(out3[0].item() - loss.item()) / E_loss}
    print(f"\n[loss-path] chain: " + " ".join(f"{k_} {v_:.3f}" for k_, v_ in ratios.items()))
    _record("chain", ratios, dev)
    assert torch.equal(hd.grad[mask.view(M) == 0], torch.zeros_like(hd.grad[mask.view(M) == 0]))
    assert (dh.cpu()[mask.view(M) == 0] == 0).all()                   # masked tokens: coef = 0, rows exactly zero
    assert ratios["dh"] <= MARGIN["dh"] and ratios["loss"] <= 1.0, ratios
