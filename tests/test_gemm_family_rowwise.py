"""The kernels that carry the step's FLOPs — k_gemm.hip (bra_gemm_bf16_nt on every kernel body, the skinny kernel, split-K, the SwiGLU
epilogue, the fp8 kernel), k_wgrad.hip and k_lora.hip — element by element against float64 statements of the same operations.

tests/test_kernels.py, tests/test_fp8_gemm.py and tests/test_lora_ranks.py bound one Frobenius ratio per output tensor (4e-3 for bf16,
1e-5 for fp32 outputs).  One K-tile dropped on one edge tile, the LoRA pair skipped for the last tile row, a residual read at the wrong
pitch for 16 rows, a split-K slice that loses its tail, a row of fp8 scales shifted by one: each moves a few rows by a few per cent and
passes there.  Here every element is held, on two kinds of value set:

  exact   operands are small integers (|a|, |b| <= 4; e4m3 integers <= 8 for the fp8 kernel), bias / residual / the accumulated-into C
          integers <= 256, alpha (and the fp8 row / column scales, and the dropout keep scale 1 / (1 - 0.5) = 2) powers of two.  With
          K + K2 <= 2624 every partial sum is below 16 * 2624 < 2^24: an exact fp32 number in ANY accumulation order, inside any MFMA,
          through any atomic add.  fp32 outputs equal the float64 result bit for bit; bf16 outputs equal the float64 result rounded once
          to bf16 — and a second time after the residual add, rnd(rnd(alpha acc + bias) + res), as the EPI_BF16 comment states.  Element
          (1, 3) of every product with more than one row is planted at 257 (x alpha: a tie between two bf16 numbers) and the integer bias moves many
          more sums onto ties: round-to-nearest-even runs in pack_bf2 and in the scalar f2bf tail (asserted: `ties`).  No tolerance.
  random  N(0, 0.5) bf16 operands, alpha = 0.3125 (a LoRA scale lora_alpha / r = 10 / 32: not a power of two), real bias / residual.
          Each element under a first-order bound, never fitted:

              err <= MARGIN[what] * E           MARGIN[what] = 2 x TWIN_WORST[what]

          fp32 outputs   E = (K + K2 + c) u S,   u = 2^-24,   S = |alpha| sum_k |a_mk| |b_nk|  (+ |bias_n|) (+ |C_mn| when accumulating)
              a product of two bf16 numbers is exact in fp32; a sum of K + K2 of them in any order is within (K + K2 - 1) u S of the
              exact one to first order; c counts the epilogue's own roundings, each relative to a partial result <= S:
                bra_gemm_bf16_nt   c = 3   acc * alpha, + bias, + C (accumulate); alpha itself is handed to the reference as the fp32 number
                                           the kernel receives
                split-K            c = 1 + split_k   acc * alpha per slice, one atomic add per slice
                skinny kernel      c = 3 + 3   the four waves' partial tiles meet in three more additions
                fp8 kernel         c = 2   acc * sa[m], * sb[n]  (K = fp8 elements; products of two e4m3 numbers are exact in fp32)
                wgrad              c = 2 + chunks   (K := M rows); alpha * acc, the masked operand's keep scale 1 / (1 - p) as an fp32
                                           number, one atomic add per row chunk
                lora_down          c = 2   alpha * acc, the keep scale
                lora_up            c = 2   (K := the group's rank columns) the keep scale as an fp32 number, its product with the sum
          bf16 outputs   + U |v| per bf16 rounding point, U = 2^-9 (tests/test_attn_rowwise.py: half of bf16's worst-case relative
              rounding error, so a maximum over 10^5 elements sits just under 2 and MARGIN just under 4);
              residual form  + U |rnd(v)| + U |out|;
              masked LoRA operand  + U |alpha| sum_k |xd_mk| |a_rk|: drop_apply8 rounds keep / (1 - p) * x to bf16 before the MFMA
              (as torch's dropout on a bf16 tensor does): a rounding point of the twin.
          Dropped elements: lora_up's output is an exact zero where every target's mask is zero — the reference is zero there and a
          non-zero value is an infinite ratio (_ratio's convention).
          fp8 on the device: v_mfma_scale_f32_16x16x128_f8f6f4 does not sum its 128 products exactly — they are aligned to a common exponent and
          truncated inside the instruction.  tools/fp8_accum_probe.py measured that on the bare instruction (profiles/r6_r_fp8_accum_probe.txt:
          at most 1.474e-4 x sum |products| over all e4m3 codes at K = 128, less at larger K).  This is the instruction's arithmetic, not the
          kernel's: FP8_MFMA_ALIGN x S is subtracted from the error BEFORE the ratio is formed, on the device only (the emulator sums in
          fp32).  Integer products <= 64 lie within 7 bits of each other: the exact set stays bit for bit on both legs.

The rounding twin (no project code): float32 torch with sequential accumulation over k (first pair, then the LoRA pair), the epilogue's
operations one by one, .to(bfloat16) at every rounding point.  The factor 2 covers what it does not model: accumulation order inside
and across MFMAs, four waves' partial tiles, atomics, -ffast-math contraction of a product and a sum.  test_twin_ratio_is_the_recorded_one
measures TWIN_WORST again on a CPU.

Every output is a window of a taller, wider buffer pre-filled with a pattern; after the call everything outside [M, N] still holds it:
"rows past M are computed and never stored" is asserted for every case here.  The window starts at column 8 of rows of a pitch that is
a multiple of 8 (`lds`: 16-byte aligned rows, the epilogue that turns a wave's block through LDS applies) or at column 4 of rows whose
pitch is 4 mod 8 (`direct`: epi_bf16_interior's 8-byte stores); a residual whose pitch is not a multiple of 4 sends every wave through
the generic epilogue (`odd`).  The three must agree bit for bit — on the exact set AND on the random set (epi_scale_bias exists for that).

Kernel bodies are pinned with bra_gemm_set_variant (emulator / debug library): 0 - 3 register-staged (128 / 256 rows x prefetch 1 / 2),
5 / 9 / 10 LDS-DMA at 256 / 192 / 128 rows, 6 / 7 four- / two-phase ring (256 x 256), 11 - 14 the four-wave kernel at 160 x 256, 128 x 256,
160 x 128, 128 x 128.  K % 64 != 0 takes the BK = 32 instance of gemm_nt_kernel whatever is pinned; variants 0 - 3 differ there.  The fp8
tile heights are pinned with bra_gemm_set_glds_rows.  What the product library chooses by itself is asserted through the dispatch mirror
of tests/test_loss_path_rowwise.py (_route_bf16) on the device: one shape per route, exact values, float64 reference on the GPU.
"""
import functools
import json
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bioreason_amd import ops, _lib                                  # noqa: E402
from test_loss_path_rowwise import _route_bf16, W4_TILES             # noqa: E402
from test_lora_ranks import RANK_CASES, r_pad                        # noqa: E402

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0 ** -9
U32 = 2.0 ** -24
ALPHA_EXACT = 0.5
ALPHA_RAND = 0.3125
FP8_MFMA_ALIGN = 1.474e-4          # profiles/r6_r_fp8_accum_probe.txt, "K 128 all codes": the instruction's own worst error / sum |products|

# The rounding twin's worst err / E per quantity over the module's random cases (CPU) and the case that reached it.
TWIN_WORST = {
    "f32": 0.0103,          # 162x259x128+64, fp32 + bias + accumulate (the bound is the worst case of K + K2 aligned roundings; a sum's actual error grows like its root)
    "bf16": 1.9393,         # 130x132x128+64, bias: one bf16 rounding, worst case 2 U, among 10^4 elements
    "res": 1.9636,          # 130x259x64, residual
    "fp8_f32": 0.0082,      # 194x131x128
    "fp8_bf16": 1.9456,     # 258x132x384, residual
    "wgrad": 0.0509,        # 33x136x192 in two row chunks: each chunk's atomic add into C rounds at the magnitude of C
    "wgrad_drop": 0.689,    # r = 32 x 2 targets (the masked operand's bf16 rounding carries the bound)
    "lora_down": 0.7476,    # r = 32 x 3 targets, 70x136
    "lora_up": 1.981,       # r = 8 x 3 targets, 70x136
}
MARGIN = {k_: 2 * v_ for k_, v_ in TWIN_WORST.items()}

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIO_FILE = os.path.join(os.environ.get("BRA_TEST_EVIDENCE_DIR") or os.path.join(ROOT, "test_evidence"), "gemm_family_rowwise_ratios.json")


# ----------------------------------------------------------------------------- helpers
def _bf(x):
    return x.to(BF).to(F64)


def _f32(x):
    return float(torch.tensor(x, dtype=F32))


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)


def _assert_bits(name, got, want):
    """got (kernel) == want (the float64 twin in the output type), bit for bit"""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, want.dtype, got.shape, want.shape)
    bad = _bits(got) != _bits(want)
    if bad.any():
        idx = torch.nonzero(bad)
        rows = sorted(set(idx[:, 0].tolist()))
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements differ, rows {rows[:6]}..{rows[-1]}, first {idx[0].tolist()}: "
                             f"got {got[tuple(idx[0])].item()} want {want[tuple(idx[0])].item()}")


def _ties(v):
    """how many elements of the float64 tensor v lie exactly half way between two bf16 numbers"""
    b = _bf(v)
    other = 2 * v - b
    return int(((v != b) & (_bf(other) == other)).sum())


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
        data = {}
    data["margin"], data["twin_worst"] = MARGIN, TWIN_WORST
    cases = data.setdefault("cases", {})
    cases[name] = {k_: round(v_, 4) for k_, v_ in ratios.items()}
    worst = {}
    for c_ in cases.values():
        for k_, v_ in c_.items():
            worst[k_] = max(worst.get(k_, 0.0), v_)
    data["worst"] = worst
    with open(RATIO_FILE, "w") as fh:
        json.dump(data, fh, indent=1)


def _assert_ratios(name, ratios, dev):
    print(f"\n[gemm-family] {name}: " + " ".join(f"{k_} {v_:.3f}" for k_, v_ in ratios.items()))
    _record(name, ratios, dev)
    for k_, v_ in ratios.items():
        assert v_ <= MARGIN[k_], (name, k_, v_, MARGIN[k_])


def _pattern(rows, cols, dtype):
    i, j = torch.arange(rows)[:, None], torch.arange(cols)[None, :]
    return (((i * 7 + j * 3) % 61) - 30).to(dtype)


class _Window:
    """an [M, N] window of a taller, wider buffer that holds a pattern of integers (|.| <= 30); layout `lds`: the window starts at column 8,
    pitch % 8 == 0; `direct`: column 4, pitch % 8 == 4.  `init` replaces the window's own pattern (the accumulating forms)"""

    def __init__(self, M, N, dtype, dev, layout="lds", init=None):
        self.M, self.N = M, N
        self.off = 8 if layout == "lds" else 4
        ld = -(-(N + self.off + 1) // 8) * 8 + (0 if layout == "lds" else 4)
        buf = _pattern(M + 3, ld, dtype)
        if init is not None:
            buf[1:1 + M, self.off:self.off + N] = init.to(dtype)
        self.buf = buf.to(dev)
        self.before = buf.clone()
        self.win = self.buf[1:1 + M, self.off:self.off + N]
        assert self.win.stride(0) % 4 == 0 and (layout != "lds" or (self.win.stride(0) % 8 == 0 and self.win.data_ptr() % 16 == 0))

    def start(self):
        """the window's contents before the call, float64 on the CPU"""
        return self.before[1:1 + self.M, self.off:self.off + self.N].to(F64)

    def result(self, name):
        """the window after the call (CPU); everything around it must still hold the pattern"""
        after = self.buf.detach().cpu().clone()
        got = after[1:1 + self.M, self.off:self.off + self.N].clone()
        ref = self.before.clone()
        after[1:1 + self.M, self.off:self.off + self.N] = 0
        ref[1:1 + self.M, self.off:self.off + self.N] = 0
        bad = _bits(after) != _bits(ref)
        assert not bad.any(), f"{name}: {int(bad.sum())} elements outside the [M, N] window were written, first at {torch.nonzero(bad)[0].tolist()} (window rows 1.., columns {self.off}..)"
        return got


def _wide(t, dev):
    """t as a column slice of a wider tensor whose other columns hold NaN"""
    w = torch.full((t.shape[0], t.shape[1] + 24), float("nan"), dtype=t.dtype)
    w[:, 8:8 + t.shape[1]] = t
    return w.to(dev)[:, 8:8 + t.shape[1]]


def _odd_pitch(t, dev):
    """t as the first columns of a tensor two columns wider: a row pitch that is not a multiple of 4"""
    w = torch.full((t.shape[0], t.shape[1] + 2), float("nan"), dtype=t.dtype)
    w[:, :t.shape[1]] = t
    v = w.to(dev)[:, :t.shape[1]]
    assert v.stride(0) % 4 != 0
    return v


def _randint(g, shape, a):
    return torch.randint(-a, a + 1, shape, generator=g).to(F64)


def _seq_matmul32(a, b):
    """float32 a [M, K] @ b [N, K]^T accumulated one k after the other (the twin's accumulation order)"""
    a, b = a.to(F32), b.to(F32)
    acc = torch.zeros(a.shape[0], b.shape[0], dtype=F32)
    bt = b.T.contiguous()
    for k in range(a.shape[1]):
        acc = acc + a[:, k, None] * bt[k][None, :]
    return acc


# ----------------------------------------------------------------------------- bra_gemm_bf16_nt: operands, reference, twin
@functools.lru_cache(maxsize=None)
def _gemm_inputs(M, N, K, K2, vals):
    """bf16 operands on the CPU and the float64 products they define.  exact: integers, rows and columns all different, the planted 257"""
    g = torch.Generator().manual_seed(100003 * M + 1009 * N + 7 * K + K2 + (0 if vals == "exact" else 1))
    d = {"M": M, "N": N, "K": K, "K2": K2, "vals": vals}
    if vals == "exact":
        assert K + K2 <= 2624
        a, b = _randint(g, (M, K), 4), _randint(g, (N, K), 4)
        a2, b2 = _randint(g, (M, K2), 4), _randint(g, (N, K2), 4)
        if M > 1:                                                                           # (a single row stays a full random row)
            a[1], b[3], a2[1] = 0, 0, 0
            a[1, :16], b[3, :16], a[1, 16], b[3, 16] = 4, 4, 1, 1                           # 16 * 16 + 1 = 257
        bias, res, c0_ = _randint(g, (N,), 256), _randint(g, (M, N), 256), _randint(g, (M, N), 256)
        ab, bb = torch.cat([a, a2], 1), torch.cat([b, b2], 1)
        assert torch.unique(ab, dim=0).shape[0] == M and torch.unique(bb, dim=0).shape[0] == N
    else:
        a, b = torch.randn(M, K, generator=g) * 0.5, torch.randn(N, K, generator=g) * 0.5
        a2, b2 = torch.randn(M, K2, generator=g) * 0.5, torch.randn(N, K2, generator=g) * 0.5
        bias, res, c0_ = torch.randn(N, generator=g), torch.randn(M, N, generator=g), torch.randn(M, N, generator=g).to(F32)
    for k_, v_ in (("a", a), ("b", b), ("a2", a2), ("b2", b2), ("bias", bias), ("res", res)):
        d[k_] = v_.to(BF)
    d["c0"] = c0_.to(F32)
    A, B, A2, B2 = (d[k_].to(F64) for k_ in ("a", "b", "a2", "b2"))
    d["acc"] = A @ B.T + A2 @ B2.T
    d["sabs"] = A.abs() @ B.abs().T + A2.abs() @ B2.abs().T
    if vals == "exact":
        assert (M == 1 or d["acc"][1, 3] == 257) and d["sabs"].max() < 2 ** 24
    return d


def _gemm_ref(d, alpha, bias=False, res=False, f32=False, accumulate=False, c_epi=3, first_pair_only=False, c0=None):
    """-> (want in the output type (the exact set's expectation), float64 reference, E, quantity)"""
    al = _f32(alpha)
    acc, sabs = d["acc"], d["sabs"]
    if first_pair_only:
        A, B = d["a"].to(F64), d["b"].to(F64)
        acc, sabs = A @ B.T, A.abs() @ B.abs().T
    v, S = al * acc, abs(al) * sabs
    if bias:
        v, S = v + d["bias"].to(F64)[None, :], S + d["bias"].to(F64).abs()[None, :]
    if accumulate:
        start = (d["c0"] if c0 is None else c0).to(F64)
        v, S = v + start, S + start.abs()
    E = (d["K"] + (0 if first_pair_only else d["K2"]) + c_epi) * U32 * S
    if f32:
        return v.to(F32), v, E, "f32"
    if not res:
        return v.to(BF), v, E + U * v.abs(), "bf16"
    r = d["res"].to(F64)
    out = _bf(v) + r
    return out.to(BF), v + r, E + U * _bf(v).abs() + U * out.abs(), "res"


def _gemm_twin(d, alpha, bias=False, res=False, f32=False, accumulate=False, first_pair_only=False, c0=None):
    """float32 restatement: sequential k, acc * alpha, + bias, (+ C), bf16, (+ res, bf16)"""
    acc = _seq_matmul32(d["a"], d["b"])
    if not first_pair_only and d["K2"]:
        a2, b2 = d["a2"].to(F32), d["b2"].to(F32).T.contiguous()
        for k in range(d["K2"]):
            acc = acc + a2[:, k, None] * b2[k][None, :]
    v = acc * torch.tensor(alpha, dtype=F32)
    if bias:
        v = v + d["bias"].to(F32)[None, :]
    if accumulate:
        v = v + (d["c0"] if c0 is None else c0).to(F32)
    if f32:
        return v
    v = v.to(BF)
    if res:
        v = (v.to(F32) + d["res"].to(F32)).to(BF)
    return v


def _gemm_call(dev, d, alpha, bias=False, res=False, f32=False, accumulate=False, layout="lds", strided=False, name=""):
    """ops.gemm_nt into a window; res: False | True | "odd" (pitch not a multiple of 4).  -> the window (CPU)"""
    M, N = d["M"], d["N"]
    put = (lambda t: _wide(t, dev)) if strided else (lambda t: t.to(dev))
    a, b = put(d["a"]), d["b"].to(dev)
    a2 = put(d["a2"]) if d["K2"] else None
    b2 = d["b2"].to(dev) if d["K2"] else None
    r = None
    if res:
        r = _odd_pitch(d["res"], dev) if res == "odd" else put(d["res"])
    win = _Window(M, N, F32 if f32 else BF, dev, layout, init=d["c0"] if accumulate else None)
    ops.gemm_nt(a, b, a2=a2, b2=b2, bias=d["bias"].to(dev) if bias else None, res=r, out=win.win, alpha=alpha, out_f32=f32, accumulate=accumulate)
    return win.result(name)


FORMS = {"plain": {}, "bias": {"bias": True}, "res": {"res": True}, "bias+res": {"bias": True, "res": True},
         "f32": {"f32": True}, "f32+bias": {"f32": True, "bias": True}, "f32+bias+acc": {"f32": True, "bias": True, "accumulate": True},
         "f32+acc": {"f32": True, "accumulate": True}}


def _check_gemm(dev, name, d, form, ratios, c_epi=3, **call_kw):
    """one call of one form: bit for bit on the exact set, under the bound on the random set (worst ratio per quantity into `ratios`).
    -> (the window, (ties among the bf16 rounding inputs, ties among those of the ragged quad's columns))"""
    kw = dict(FORMS[form])
    exact = d["vals"] == "exact"
    alpha = ALPHA_EXACT if exact else ALPHA_RAND
    got = _gemm_call(dev, d, alpha, name=name, **kw, **call_kw)
    want, ref, E, what = _gemm_ref(d, alpha, c_epi=c_epi, **kw)
    if exact:
        _assert_bits(f"{name} [{form}]", got, want)
        if kw.get("f32"):
            return got, (0, 0)
        pre = ref - d["res"].to(F64) if kw.get("res") else ref      # what the first bf16 rounding sees
        N = d["N"]
        return got, (_ties(pre), _ties(pre[:, N - N % 4:]) if N % 4 else 0)
    assert not torch.isnan(got.float()).any(), name
    ratios[what] = max(ratios.get(what, 0.0), _ratio((got.to(F64) - ref).abs(), E))
    return got, (0, 0)


# variant: (rows, columns) of its tile
TILE = {0: (128, 128), 1: (128, 128), 2: (256, 128), 3: (256, 128), 5: (256, 128), 9: (192, 128), 10: (128, 128), 6: (256, 256), 7: (256, 256),
        11: (160, 256), 12: (128, 256), 13: (160, 128), 14: (128, 128)}
VARIANTS = list(TILE)


def _pinned(variant):
    class _Pin:
        def __enter__(self):
            _lib.get_lib().call("bra_gemm_set_variant", variant)

        def __exit__(self, *exc):
            _lib.get_lib().call("bra_gemm_set_variant", -1)
    return _Pin()


def _bodies_cases(variant, vals):
    """(M, N, K, K2, form, call options) of one kernel body: a full tile plus a ragged one in M (BM + 2) and N (BN + 4; BN + 3: the ragged
    quad), a single K-tile, both operand pairs, the LoRA pair the longer one; K % 64 != 0 where the pinned body changes the kernel"""
    bm, bn = TILE[variant]
    M, N4, N3 = bm + 2, bn + 4, bn + 3
    if vals == "exact":
        cases = [(M, N4, 64, 0, f, {}) for f in ("plain", "bias", "res", "bias+res", "f32", "f32+bias+acc")]
        cases += [(M, N4, 64, 0, "bias+res", {"layout": "direct"}), (M, N4, 64, 0, "res", {"layout": "direct"}),
                  (M, N3, 128, 64, "bias+res", {"strided": True}), (M, N3, 128, 64, "f32+acc", {}), (M, N3, 64, 0, "plain", {"layout": "direct"}),
                  (M, N4, 64, 128, "bias+res", {}), (M, N4, 64, 128, "f32+bias", {"strided": True})]
        if variant <= 3:
            cases += [(M, N3, 32, 0, "bias+res", {}), (M, N4, 96, 32, "f32+bias+acc", {}), (M, N4, 32, 96, "bias", {"strided": True})]
        return cases
    cases = [(M, N4, 128, 64, "bias+res", {}), (M, N4, 128, 64, "bias", {"layout": "direct"}), (M, N3, 128, 64, "f32+bias+acc", {"strided": True}),
             (M, N3, 64, 0, "res", {})]
    if variant <= 3:
        cases += [(M, N4, 96, 32, "bias+res", {})]
    return cases


def _run_bodies(dev, variant, vals):
    ratios, ties = {}, [0, 0]
    with _pinned(variant):
        for (M, N, K, K2, form, opt) in _bodies_cases(variant, vals):
            d = _gemm_inputs(M, N, K, K2, vals)
            name = f"v{variant}-{M}x{N}x{K}+{K2}-{vals}" + "".join(f"-{k_}" for k_ in opt)
            got, t = _check_gemm(dev, name, d, form, ratios, **opt)
            ties = [ties[0] + t[0], ties[1] + t[1]]
            if FORMS[form].get("res") and N % 4 == 0 and "strided" not in opt:
                # interior (LDS-turned or direct) and generic epilogue: the same bits, whatever the values
                kw = dict(FORMS[form])
                kw["res"] = "odd"
                alpha = ALPHA_EXACT if vals == "exact" else ALPHA_RAND
                odd = _gemm_call(dev, d, alpha, name=name + "-odd", layout=opt.get("layout", "lds"), **kw)
                _assert_bits(name + f" [{form}]: generic epilogue (residual pitch % 4 != 0) against the interior one", odd, got)
    return ratios, ties


# ----------------------------------------------------------------------------- 1: every kernel body
@pytest.mark.parametrize("variant", VARIANTS)
def test_gemm_bodies_exact(debug_backend, variant):
    """bit for bit against the float64 twin: tile edges in M and N, the ragged quad (N % 4 = 3 through a sliced out), one K-tile, both
    operand pairs, every bias / residual combination, fp32 with and without accumulate, strided A / A2 / res, three epilogue routes"""
    _, ties = _run_bodies(debug_backend, variant, "exact")
    assert ties[0] > 0 and ties[1] > 0, f"no sum landed on a bf16 tie (pack_bf2, the scalar f2bf tail): {ties}"


@pytest.mark.parametrize("variant", VARIANTS)
def test_gemm_bodies_random(debug_backend, variant):
    """every element under its first-order bound; interior and generic epilogue agree bit for bit on real values too"""
    ratios, _ = _run_bodies(debug_backend, variant, "rand")
    _assert_ratios(f"bodies-v{variant}", ratios, debug_backend)


# ----------------------------------------------------------------------------- 2: the skinny kernel
SKINNY_K = 2 * 1024 + 96        # 67 steps of 32: waves 0 - 2 run the eight-in-flight loop twice and the tail once, wave 3 twice and no tail
SKINNY = [(M, N, K2) for M in (1, 5, 16) for N in (8, 40, 131, 144) for K2 in (0, 64)]


def _skinny_forms(M, N, K2):
    i = (M + N + K2 // 64) % 2
    return (("bias+res", "f32+bias+acc") if i else ("res", "f32+acc")) + (("plain",) if N == 131 else ()) + (("f32+bias",) if M == 5 else ())


@pytest.mark.parametrize("M,N,K2", SKINNY)
def test_gemm_skinny_exact(backend, M, N, K2):
    """gemm_skinny_kernel (M <= 16): the deep loop, the row clamp (M < 16) and the column clamp (N % 16 != 0) together, the ragged quad
    (N = 131 through a slice), the LoRA pair, every epilogue form across the cases; K + K2 = 2208 <= 2624: bit for bit"""
    assert _route_bf16(M, N, SKINNY_K, K2) == "skinny"
    d = _gemm_inputs(M, N, SKINNY_K, K2, "exact")
    ties = 0
    for form in _skinny_forms(M, N, K2):
        ties += _check_gemm(backend, f"skinny-{M}x{N}x{SKINNY_K}+{K2}", d, form, {}, strided=(N == 40))[1][0]
    assert ties > 0 or M * N < 64


@pytest.mark.parametrize("M,N,K2", [(1, 131, 64), (5, 40, 0), (5, 144, 64), (16, 131, 0), (16, 8, 64)])
def test_gemm_skinny_random(backend, M, N, K2):
    d = _gemm_inputs(M, N, SKINNY_K, K2, "rand")
    ratios = {}
    for form in ("bias+res", "f32+bias+acc", "bias"):
        _check_gemm(backend, f"skinny-{M}x{N}x{SKINNY_K}+{K2}-rand", d, form, ratios, c_epi=6)
    _assert_ratios(f"skinny-{M}x{N}+{K2}", ratios, backend)


# ----------------------------------------------------------------------------- 3: split-K
# (K, split_k): 5 K-tiles in 3 slices (2 + 2 + 1: the last slice is short), 8 slices for 5 tiles (three workgroups return empty),
# 3 tiles in 2 slices; K = 96 is three K-tiles of the BK = 32 instance
SPLITK = [(320, 3), (320, 8), (192, 2), (96, 2)]


def _splitk_case(dev, variant, K, split_k, vals, ratios):
    M, N = 130, 131
    d = _gemm_inputs(M, N, K, 0, vals)
    exact = vals == "exact"
    alpha = 2.0 if exact else ALPHA_RAND
    win = _Window(M, N, F32, dev, "direct")
    c0 = win.start()
    name = f"splitk-v{variant}-{K}/{split_k}-{vals}"
    ops.gemm_nt_splitk(_wide(d["a"], dev), d["b"].to(dev), win.win, alpha=alpha, split_k=split_k)
    got = win.result(name)
    want, ref, E, _ = _gemm_ref(d, alpha, f32=True, accumulate=True, c_epi=1 + split_k, c0=c0)
    if exact:
        _assert_bits(name, got, want)
    else:
        ratios["f32"] = max(ratios.get("f32", 0.0), _ratio((got.to(F64) - ref).abs(), E))


@pytest.mark.parametrize("variant", [0, 2, 5, 10])
def test_gemm_splitk(debug_backend, variant):
    """bra_gemm_bf16_nt_splitk on the register-staged and the LDS-DMA body, accumulating into a non-zero C through atomics: a short last
    slice, more slices than K-tiles; exact sets are bit for bit in whatever order the atomics land"""
    ratios = {}
    with _pinned(variant):
        for (K, split_k) in SPLITK:
            _splitk_case(debug_backend, variant, K, split_k, "exact", ratios)
        _splitk_case(debug_backend, variant, 320, 3, "rand", ratios)
    _assert_ratios(f"splitk-v{variant}", ratios, debug_backend)


# ----------------------------------------------------------------------------- 4: the SwiGLU epilogue
def _bf_step(b, up):
    """the bf16 number after (up) / before b, as float64"""
    i = b.to(BF).view(torch.int16).to(torch.int32)
    j = torch.where((b > 0) == up, i + 1, i - 1).to(torch.int16)
    return j.view(BF).to(F64)


@functools.lru_cache(maxsize=None)
def _swiglu_inputs(M, F, K, K2):
    """x, a2 in {+-1, +-2, +-4}; gate rows of W with four, of B2 with two entries +-1 (|g| <= 24, an integer); up rows of W one entry
    +-{1, 2, 4}, of B2 zero: u = +-2^k, so bf16(silu(g)) * u is exact and an inner flip of silu(g) would be the only way to differ"""
    g = torch.Generator().manual_seed(31 * M + F + K + K2)

    def pow2(shape):
        return (2.0 ** torch.randint(0, 3, shape, generator=g).to(F64)) * (torch.randint(0, 2, shape, generator=g).to(F64) * 2 - 1)

    def sparse(rows, cols, n):
        w = torch.zeros(rows, cols, dtype=F64)
        for i in range(n):
            c = torch.randint(0, cols, (rows,), generator=g)
            w[torch.arange(rows), c] = (torch.randint(0, 2, (rows,), generator=g) * 2 - 1).to(F64)
        return w
    x, a2 = pow2((M, K)), pow2((M, K2))
    W, B2 = torch.zeros(2 * F, K, dtype=F64), torch.zeros(2 * F, K2, dtype=F64)
    W[:F] = sparse(F, K, 4)
    W[F:] = sparse(F, K, 1) * pow2((F, 1))
    if K2:
        B2[:F] = sparse(F, K2, 2)
    return x.to(BF), W.to(BF), a2.to(BF), B2.to(BF)


@pytest.mark.parametrize("M,F,K,K2", [(257, 128, 64, 0), (257, 256, 128, 64), (257, 128, 64, 64), (40, 256, 192, 0)])
def test_gemm_swiglu_twin(backend, M, F, K, K2):
    """bra_gemm_swiglu_bf16_nt: one full 256-row tile + 1, F = 128 / 256, with and without the rank part — bit for bit against
    rnd(rnd(silu(rnd(g))) * rnd(u)) in float64 (the EPI_SWIGLU comment's rounding points) and against the two-launch form"""
    dev = backend
    x, W, a2, B2 = _swiglu_inputs(M, F, K, K2)
    gu = x.to(F64) @ W.to(F64).T + a2.to(F64) @ B2.to(F64).T
    gt, up = gu[:, :F], gu[:, F:]
    assert torch.equal(_bf(gt), gt) and gt.abs().max() <= 24 and (up != 0).all()
    assert torch.equal(torch.log2(up.abs()), torch.log2(up.abs()).round())                  # u = +-2^k
    silu = gt / (1.0 + torch.exp(-gt))
    # no gate value sits near a bf16 rounding boundary of silu: further than 16 x the fp32 chain's error (1.5 |g| + 6) u |silu|
    b = _bf(silu)
    mid = torch.minimum((silu - (b + _bf_step(b, True)) / 2).abs(), (silu - (b + _bf_step(b, False)) / 2).abs())
    nz = silu != 0
    assert (mid[nz] > 16 * (1.5 * gt[nz].abs() + 6) * U32 * silu[nz].abs()).all()
    want = (b * up).to(BF)
    assert torch.equal(want.to(F64), b * up)
    win = _Window(M, F, BF, dev, "lds")
    xd, Wd = _wide(x, dev), W.to(dev)
    a2d, B2d = (a2.to(dev), B2.to(dev)) if K2 else (None, None)
    rc = _lib.get_lib().call_rc("bra_gemm_swiglu_bf16_nt", xd, xd.stride(0), Wd, Wd.stride(0), a2d, a2d.stride(0) if K2 else 0, B2d,
                                B2d.stride(0) if K2 else 0, K2, win.win, win.win.stride(0), M, F, K, 1.0, _lib.current_stream(xd))
    assert rc == 0
    name = f"swiglu-{M}x{F}x{K}+{K2}"
    got = win.result(name)
    _assert_bits(name, got, want)
    two = ops.swiglu_fwd(ops.gemm_nt(xd, Wd, a2=a2d, b2=B2d))
    _assert_bits(name + ": the two-launch form", two, got)


# ----------------------------------------------------------------------------- 5: the fp8 kernel
def _e4m3(x):
    return x.to(F32).to(torch.float8_e4m3fn).view(torch.uint8)


def _decode(q):
    return q.view(torch.float8_e4m3fn).to(F64)


@functools.lru_cache(maxsize=None)
def _fp8_inputs(M, N, K, vals):
    g = torch.Generator().manual_seed(977 * M + 13 * N + K + (0 if vals == "exact" else 1))
    if vals == "exact":
        a8, b8 = _e4m3(_randint(g, (M, K), 8)), _e4m3(_randint(g, (N, K), 8))
        # powers of two that differ from row to row and from column to column, periods 5 and 7: no shift by one goes unnoticed
        sa = 2.0 ** ((torch.arange(M) % 5) - 2).to(F32)
        sb = 2.0 ** ((torch.arange(N) * 3 % 7) - 3).to(F32)
        res = _randint(g, (M, N), 256).to(BF)
        assert (sb[1:] != sb[:-1]).all() and (sa[1:] != sa[:-1]).all()
    else:
        a8 = torch.randint(0, 256, (M, K), generator=g, dtype=torch.int32)
        b8 = torch.randint(0, 256, (N, K), generator=g, dtype=torch.int32)
        # no NaN codes, the exponent's top bit cleared (|v| <= 1.875) as tests/test_fp8_gemm.py has it
        a8 = (torch.where((a8 & 0x7f) == 0x7f, a8 & 0x80, a8) & 0xbf).to(torch.uint8)
        b8 = (torch.where((b8 & 0x7f) == 0x7f, b8 & 0x80, b8) & 0xbf).to(torch.uint8)
        sa, sb = torch.rand(M, generator=g) + 0.5, torch.rand(N, generator=g) * 0.1 + 0.01
        res = torch.randn(M, N, generator=g).to(BF)
    A, B = _decode(a8), _decode(b8)
    sc = sa.to(F64)[:, None] * sb.to(F64)[None, :]
    return {"a8": a8, "b8": b8, "sa": sa.to(F32), "sb": sb.to(F32), "res": res, "v": (A @ B.T) * sc, "S": (A.abs() @ B.abs().T) * sc,
            "M": M, "N": N, "K": K, "vals": vals}


def _fp8_twin(d, res, f32):
    acc = _seq_matmul32(_decode(d["a8"]), _decode(d["b8"]))
    v = acc * d["sa"][:, None] * d["sb"][None, :]
    if f32:
        return v
    v = v.to(BF)
    return (v.to(F32) + d["res"].to(F32)).to(BF) if res else v


def _fp8_ref(d, res, f32):
    v, E = d["v"], (d["K"] + 2) * U32 * d["S"]
    if f32:
        return v.to(F32), v, E, "fp8_f32"
    if not res:
        return v.to(BF), v, E + U * v.abs(), "fp8_bf16"
    out = _bf(v) + d["res"].to(F64)
    return out.to(BF), v + d["res"].to(F64), E + U * _bf(v).abs() + U * out.abs(), "fp8_bf16"


def _fp8_check(dev, d, res, f32, layout, ratios, tag):
    M, N = d["M"], d["N"]
    win = _Window(M, N, F32 if f32 else BF, dev, layout)
    r = (_odd_pitch(d["res"], dev) if res == "odd" else d["res"].to(dev)) if res else None
    ops.gemm_fp8_nt(d["a8"].to(dev), d["sa"].to(dev), d["b8"].to(dev), d["sb"].to(dev), res=r, out=win.win, out_f32=f32)
    name = f"fp8-{tag}-{M}x{N}x{d['K']}-{d['vals']}" + ("-res" if res else "") + ("-f32" if f32 else "")
    got = win.result(name)
    want, ref, E, what = _fp8_ref(d, bool(res), f32)
    if d["vals"] == "exact":
        _assert_bits(name, got, want)
        return
    err = (got.to(F64) - ref).abs()
    if dev.type == "cuda":
        err = (err - FP8_MFMA_ALIGN * d["S"]).clamp_min(0)            # the instruction's own alignment error (module docstring)
    ratios[what] = max(ratios.get(what, 0.0), _ratio(err, E))


FP8_ROWS = [128, 192, 256]


def _fp8_cases(rows, vals):
    """(M, N, K, res, f32, layout) at one tile height: a full tile + 2 rows, 128 + 4 and 128 + 3 columns, one and three K-tiles"""
    M = rows + 2
    if vals == "exact":
        return [(M, 132, 128, True, False, "lds"), (M, 132, 128, "odd", False, "lds"), (M, 131, 384, False, True, "lds"), (M, 132, 384, False, False, "direct"),
                (M, 131, 128, True, False, "direct"), (M, 132, 384, False, True, "lds")]
    return [(M, 132, 384, True, False, "lds"), (M, 131, 128, False, True, "lds"), (M, 131, 384, False, False, "direct")]


@pytest.mark.parametrize("rows", FP8_ROWS)
@pytest.mark.parametrize("vals", ["exact", "rand"])
def test_gemm_fp8_rowwise(debug_backend, rows, vals):
    """bra_gemm_fp8_nt at MI = 2 / 3 / 4 (bra_gemm_set_glds_rows): e4m3 integers and power-of-two sa / sb that differ per row and per
    column bit for bit; random codes against the float64 product of the decoded bytes times the scales"""
    lib = _lib.get_lib()
    ratios = {}
    try:
        lib.call("bra_gemm_set_glds_rows", rows)
        for (M, N, K, res, f32, layout) in _fp8_cases(rows, vals):
            _fp8_check(debug_backend, _fp8_inputs(M, N, K, vals), res, f32, layout, ratios, f"r{rows}")
    finally:
        lib.call("bra_gemm_set_glds_rows", 0)
    if vals == "rand":
        _assert_ratios(f"fp8-r{rows}", ratios, debug_backend)


# ----------------------------------------------------------------------------- 6: wgrad
# (M, N, R, m_chunk): R = 192 is walked in two slices; N = 8 is narrower than one wave's 32 columns, 136 one tile + 8; m_chunk 64 / 96 / 32
# leave a short last chunk of 1 / 65 / 1 rows, 512 is larger than M, 0 = the entry point's own choice (256: 257 rows leave a chunk of one)
WGRAD = [(257, 136, 32, 64), (257, 264, 64, 96), (33, 8, 128, 0), (257, 8, 192, 512), (33, 136, 192, 32), (257, 264, 128, 0), (33, 264, 32, 512)]


def _chunk_rows(M, N, m_chunk):
    """rows per workgroup as bra_wgrad_tn states them: m_chunk rounded up to 32; 0 = enough workgroups to fill the chip twice, 256 rows at least"""
    if m_chunk <= 0:
        splits = -(-512 // -(-N // 128))
        m_chunk = max(-(-M // splits), 256)
    return -(-m_chunk // 32) * 32


def _n_chunks(M, N, m_chunk):
    return -(-M // _chunk_rows(M, N, m_chunk))


@functools.lru_cache(maxsize=None)
def _wgrad_inputs(M, N, R, vals):
    g = torch.Generator().manual_seed(M + 31 * N + 7 * R + (0 if vals == "exact" else 1))
    if vals == "exact":
        y, t = _randint(g, (M, N), 4), _randint(g, (M, R), 4)
    else:
        y, t = torch.randn(M, N, generator=g) * 0.5, torch.randn(M, R, generator=g) * 0.5
    return y.to(BF), t.to(BF)


def _wgrad_run(dev, name, y, t, yd64, alpha, m_chunk, transposed, ratios, exact, drop=None, rank=32, strided=False, c_extra=0):
    """out (+)= alpha yd^T t into a window holding the pattern; yd64 [targets or 1][M, N]: the (masked) operand per target in float64,
    target j = columns [j rank, (j + 1) rank) of t"""
    M, N = y.shape
    R = t.shape[1]
    al = _f32(alpha)
    ref, S = torch.zeros(N, R, dtype=F64), torch.zeros(N, R, dtype=F64)
    T = t.to(F64)
    if drop is None:
        ref, S = yd64[0].T @ T, yd64[0].abs().T @ T.abs()
    else:
        for j, yj in enumerate(yd64):
            ref[:, j * rank:(j + 1) * rank] = yj.T @ T[:, j * rank:(j + 1) * rank]
            S[:, j * rank:(j + 1) * rank] = yj.abs().T @ T[:, j * rank:(j + 1) * rank].abs()
    win = _Window(R, N, F32, dev, "direct") if transposed else _Window(N, R, F32, dev, "direct")
    c0 = win.start()
    yd = _wide(y, dev) if strided else y.to(dev)
    ops.wgrad_tn(yd, t.to(dev), win.win, transposed_out=transposed, alpha=alpha, m_chunk=m_chunk, drop=drop, rank=rank)
    got = win.result(name)
    if transposed:
        got, c0 = got.T, c0.T
    want = al * ref + c0
    if exact:
        _assert_bits(name, got.contiguous(), want.to(F32))
        return
    E = (M + 2 + _n_chunks(M, N, m_chunk) + c_extra) * U32 * (abs(al) * S + c0.abs()) + (U * abs(al) * S if drop is not None else 0)
    what = "wgrad" if drop is None else "wgrad_drop"
    ratios[what] = max(ratios.get(what, 0.0), _ratio((got.to(F64) - want).abs(), E))


@pytest.mark.parametrize("M,N,R,m_chunk", WGRAD)
def test_wgrad_rowwise(backend, M, N, R, m_chunk):
    """bra_wgrad_tn: both output orientations, accumulating into a non-zero C through atomics, a strided Y"""
    ratios = {}
    for vals in ("exact", "rand"):
        y, t = _wgrad_inputs(M, N, R, vals)
        for transposed in (False, True):
            _wgrad_run(backend, f"wgrad-{M}x{N}x{R}-c{m_chunk}-{vals}" + ("-T" if transposed else ""), y, t, [y.to(F64)],
                       2.0 if vals == "exact" else ALPHA_RAND, m_chunk, transposed, ratios, vals == "exact", strided=transposed)
    _assert_ratios(f"wgrad-{M}x{N}x{R}-c{m_chunk}", ratios, backend)


SEEDS = [5, 6, 7, 8]


def _masks(M, K, p, seeds, dev):
    """the exported keep masks (ops.dropout_mask), float64 on the CPU, one per target"""
    return [ops.dropout_mask(M, K, p, s, dev).cpu().to(F64) for s in seeds]


def _lora_operands(r, targets, M, K, vals):
    """x [M, K], the group's A image [R, K] and dts [M, R] in the LoraGroup layout: rows / columns past targets * r are zeros"""
    R = r_pad(r, targets)
    g = torch.Generator().manual_seed(1000 * r + 100 * targets + M + K + (0 if vals == "exact" else 1))
    if vals == "exact":
        x, A, dts = _randint(g, (M, K), 4), _randint(g, (R, K), 4), _randint(g, (M, R), 4)
    else:
        x, A, dts = torch.randn(M, K, generator=g) * 0.5, torch.randn(R, K, generator=g) * K ** -0.5, torch.randn(M, R, generator=g) * 0.5
    A[targets * r:] = 0
    dts[:, targets * r:] = 0
    return x.to(BF), A.to(BF), dts.to(BF)


def _drop_p(vals):
    return 0.5 if vals == "exact" else 0.25


def _masked64(x, masks, p):
    """keep_j / (1 - p) * x in float64, unrounded, per target"""
    return [x.to(F64) * mk / (1.0 - p) for mk in masks]


def _masked_twin(x, masks, p):
    """drop_apply8: x * (1.f / (1.f - p)) in fp32, one rounding to bf16, then the mask"""
    inv = torch.tensor(1.0, dtype=F32) / (torch.tensor(1.0, dtype=F32) - torch.tensor(p, dtype=F32))
    xs = (x.to(F32) * inv).to(BF)
    return [xs * mk.to(BF) for mk in masks]


@pytest.mark.parametrize("r,targets", RANK_CASES)
def test_wgrad_drop_rowwise(backend, r, targets):
    """bra_wgrad_tn_drop at every rank (R = 192 / 256 / 384: sliced), M = 70 in chunks of 32 (a last chunk of 6 rows), K = 136: exact with
    p = 0.5 (the masked operand is 2 x, an integer), random with p = 0.25 against the exported masks"""
    M, K = 70, 136
    seeds = SEEDS[:targets]
    ratios = {}
    for vals in ("exact", "rand"):
        p = _drop_p(vals)
        x, A, dts = _lora_operands(r, targets, M, K, vals)
        masks = _masks(M, K, p, seeds, backend)
        assert all(0.2 < mk.mean() < 0.95 for mk in masks) and (targets == 1 or not torch.equal(masks[0], masks[1]))
        for transposed in (True, False):
            _wgrad_run(backend, f"wgrad-drop-r{r}x{targets}-{vals}" + ("-T" if transposed else ""), x, dts, _masked64(x, masks, p),
                       2.0 if vals == "exact" else ALPHA_RAND, 32, transposed, ratios, vals == "exact", drop=(p, seeds), rank=r, c_extra=1)
    _assert_ratios(f"wgrad-drop-r{r}x{targets}", ratios, backend)


# ----------------------------------------------------------------------------- 7: lora_down_drop, lora_up_drop
def _lora_down_call(dev, name, x, A, alpha, p, seeds, rank, ks, layout="lds"):
    M, K = x.shape
    R = A.shape[0]
    lib = _lib.get_lib()
    win = _Window(M, R, BF, dev, layout)
    xd, Ad = _wide(x, dev), A.to(dev)
    part = torch.empty((ks, M, R), dtype=F32, device=dev) if ks > 1 else None
    lib.call("bra_lora_down_drop", xd, xd.stride(0), Ad, Ad.stride(0), win.win, win.win.stride(0), M, K, R, alpha, p, *ops._group(seeds, rank, R),
             part, ks, _lib.current_stream(xd))
    return win.result(name)


def _lora_down_ref(x, A, masks, p, alpha, r, targets):
    M, K = x.shape
    R = A.shape[0]
    al = _f32(alpha)
    v, S = torch.zeros(M, R, dtype=F64), torch.zeros(M, R, dtype=F64)
    for j, xj in enumerate(_masked64(x, masks, p)):
        Aj = A.to(F64)[j * r:(j + 1) * r]
        v[:, j * r:(j + 1) * r], S[:, j * r:(j + 1) * r] = al * xj @ Aj.T, abs(al) * xj.abs() @ Aj.abs().T
    return v, ((K + 2) * U32 + U) * S + U * v.abs()


def _lora_down_twin(x, A, masks, p, alpha, r, targets):
    t = torch.zeros(x.shape[0], A.shape[0], dtype=F32)
    for j, xj in enumerate(_masked_twin(x, masks, p)):
        t[:, j * r:(j + 1) * r] = _seq_matmul32(xj, A[j * r:(j + 1) * r])
    return (t * torch.tensor(alpha, dtype=F32)).to(BF)


def _lora_up_ref(dts, A, masks, p, r, targets):
    M, K = dts.shape[0], A.shape[1]
    v, S = torch.zeros(M, K, dtype=F64), torch.zeros(M, K, dtype=F64)
    D, A64 = dts.to(F64), A.to(F64)
    for j, mk in enumerate(masks):
        v += mk / (1.0 - p) * (D[:, j * r:(j + 1) * r] @ A64[j * r:(j + 1) * r])
        S += mk / (1.0 - p) * (D[:, j * r:(j + 1) * r].abs() @ A64[j * r:(j + 1) * r].abs())
    return v, (targets * r + 2) * U32 * S + U * v.abs()


def _lora_up_twin(dts, A, masks, p, r, targets):
    inv = torch.tensor(1.0, dtype=F32) / (torch.tensor(1.0, dtype=F32) - torch.tensor(p, dtype=F32))
    o = torch.zeros(dts.shape[0], A.shape[1], dtype=F32)
    for j, mk in enumerate(masks):
        o = o + _seq_matmul32(dts[:, j * r:(j + 1) * r], A[j * r:(j + 1) * r].T.contiguous()) * mk.to(F32)
    return (o * inv).to(BF)


LORA_SHAPES = [(33, 896), (70, 136)]       # K = 896: seven K steps, bra_lora_down_splitk_plan = 2; K = 136: one step + 8


def _lora_case(dev, r, targets, M, K, vals, ratios):
    seeds = SEEDS[:targets]
    p = _drop_p(vals)
    alpha = 0.5 if vals == "exact" else ALPHA_RAND
    x, A, dts = _lora_operands(r, targets, M, K, vals)
    R = A.shape[0]
    masks = _masks(M, K, p, seeds, dev)
    tag = f"r{r}x{targets}-{M}x{K}-{vals}"
    plan = int(_lib.get_lib()._dll.bra_lora_down_splitk_plan(M, K))
    assert plan == (2 if K == 896 else 1)
    v, E = _lora_down_ref(x, A, masks, p, alpha, r, targets)
    t1 = _lora_down_call(dev, "lora_down-" + tag, x, A, alpha, p, seeds, r, 1)
    assert (t1[:, targets * r:] == 0).all(), "padding columns of t must be exact zeros"
    outs = [("plain", t1)]
    if plan > 1:
        tk = _lora_down_call(dev, "lora_down-splitk-" + tag, x, A, alpha, p, seeds, r, plan, layout="direct")
        assert (tk[:, targets * r:] == 0).all()
        outs.append(("splitk", tk))
    for form, t in outs:
        if vals == "exact":
            _assert_bits(f"lora_down-{form}-{tag}", t, v.to(BF))
        else:
            ratios["lora_down"] = max(ratios.get("lora_down", 0.0), _ratio((t.to(F64) - v).abs(), E))
    if vals == "exact" and plan > 1:
        _assert_bits(f"lora_down-{tag}: split-K against plain", outs[1][1], t1)
    # the branch's input gradient
    vu, Eu = _lora_up_ref(dts, A, masks, p, r, targets)
    AT = A.T.contiguous()
    for layout in ("lds", "direct") if K == 136 else ("lds",):
        win = _Window(M, K, BF, dev, layout)
        dd, ATd = _wide(dts, dev), AT.to(dev)
        _lib.get_lib().call("bra_lora_up_drop", dd, dd.stride(0), ATd, ATd.stride(0), win.win, win.win.stride(0), M, K, R, p,
                            *ops._group(seeds, r, R), _lib.current_stream(dd))
        up = win.result(f"lora_up-{tag}-{layout}")
        dropped = torch.stack(masks).sum(0) == 0
        assert dropped.any() and (up[dropped] == 0).all(), "an element every target dropped is an exact zero"
        if vals == "exact":
            _assert_bits(f"lora_up-{tag}-{layout}", up, vu.to(BF))
        else:
            ratios["lora_up"] = max(ratios.get("lora_up", 0.0), _ratio((up.to(F64) - vu).abs(), Eu))


@pytest.mark.parametrize("r,targets", RANK_CASES)
def test_lora_drop_rowwise(backend, r, targets):
    """bra_lora_down_drop (plain and split-K) and bra_lora_up_drop at every rank and target count: M = 33 / 70 (not multiples of 32),
    K = 896 / 136; exact with p = 0.5 — the whole kernel bit for bit, split-K equal to plain — and random with p = 0.25 under the bound;
    padding columns and fully dropped elements are exact zeros"""
    ratios = {}
    for (M, K) in LORA_SHAPES:
        for vals in ("exact", "rand"):
            _lora_case(backend, r, targets, M, K, vals, ratios)
    _assert_ratios(f"lora-r{r}x{targets}", ratios, backend)


# ----------------------------------------------------------------------------- 8: the seams of automatic dispatch (device, product library)
# route: (M, N, K, K2) — the smallest shapes found with the mirror; the row split needs more than one round of 256 x 256 tiles
ROUTES = {"nt128": (130, 132, 64, 0), "nt128-bk32": (130, 132, 96, 32), "glds256": (256, 16400, 64, 0), "glds192": (384, 11100, 64, 0),
          "glds128": (256, 8200, 64, 0), "ring": (300, 17700, 64, 64), "split": (2400, 8192, 768, 0),
          "w4-1": (905, 8240, 192, 64), "w4-2": (609, 8240, 256, 0), "w4-3": (387, 8240, 256, 0), "w4-4": (130, 260, 192, 64)}


def test_dispatch_mirror_routes():
    """every device-only case takes the route written next to it, and together they are all the routes dispatch_bk has"""
    for route, shape in ROUTES.items():
        assert _route_bf16(*shape) == route.split("-bk")[0], (route, shape, _route_bf16(*shape))
    assert {_route_bf16(*s) for s in ROUTES.values()} == {"nt128", "glds256", "glds192", "glds128", "ring", "split"} | {f"w4-{c}" for c in W4_TILES}
    assert _route_bf16(16, 4096, 2048) == "skinny" and _route_bf16(17, 4096, 2048) != "skinny"
    # the step's own projections: M = 2180 rows of one prompt, N = 2048 / 6144 / 12288, K = 2048 + the rank-64 pair
    assert _route_bf16(17440, 2048, 2048, 64) in ("ring", "split")


@pytest.mark.gpu
@pytest.mark.parametrize("route", list(ROUTES))
def test_gemm_product_dispatch_exact(hip_device, route):
    """the product library's own choice of kernel, exact values, float64 reference on the GPU: bf16 + bias + residual and fp32"""
    dev = hip_device
    M, N, K, K2 = ROUTES[route]
    assert _route_bf16(M, N, K, K2) == route.split("-bk")[0]
    g = torch.Generator().manual_seed(M + N + K)
    a, b = _randint(g, (M, K), 4).to(BF).to(dev), _randint(g, (N, K), 4).to(BF).to(dev)
    a2, b2 = (_randint(g, (M, K2), 4).to(BF).to(dev), _randint(g, (N, K2), 4).to(BF).to(dev)) if K2 else (None, None)
    bias, res = _randint(g, (N,), 256).to(BF).to(dev), _randint(g, (M, N), 256).to(BF).to(dev)
    v = a.to(F64) @ b.to(F64).T
    if K2:
        v = v + a2.to(F64) @ b2.to(F64).T
    v = ALPHA_EXACT * v
    fill = torch.full((M + 2, N + 8), -7.0, device=dev)
    c32 = fill.clone()
    ops.gemm_nt(a, b, a2=a2, b2=b2, out=c32[1:1 + M, 4:4 + N], alpha=ALPHA_EXACT, out_f32=True)
    assert torch.equal(c32[1:1 + M, 4:4 + N].to(F64), v), f"{route}: fp32 output differs from float64"
    c32[1:1 + M, 4:4 + N] = -7.0
    assert torch.equal(c32, fill), f"{route}: written outside [M, N]"
    fill16 = fill.to(BF)
    c16 = fill16.clone()
    out = c16[1:1 + M, 4:4 + N]
    ops.gemm_nt(a, b, a2=a2, b2=b2, bias=bias, res=res, out=out, alpha=ALPHA_EXACT)
    want = (_bf(v + bias.to(F64)[None, :]) + res.to(F64)).to(BF)
    bad = out.view(torch.int16) != want.view(torch.int16) if out.is_contiguous() else out.contiguous().view(torch.int16) != want.view(torch.int16)
    assert not bad.any(), f"{route}: {int(bad.sum())} elements differ, first {torch.nonzero(bad)[0].tolist()}"
    c16[1:1 + M, 4:4 + N] = -7.0
    assert torch.equal(c16, fill16), f"{route}: written outside [M, N]"


# ----------------------------------------------------------------------------- the twin
def _twin_worst():
    worst, where = dict.fromkeys(TWIN_WORST, 0.0), {}

    def note(what, name, got, ref, E):
        w = _ratio((got.to(F64) - ref).abs(), E)
        if w > worst[what]:
            worst[what], where[what] = w, name

    for variant in VARIANTS:
        for (M, N, K, K2, form, opt) in _bodies_cases(variant, "rand"):
            d = _gemm_inputs(M, N, K, K2, "rand")
            kw = FORMS[form]
            _, ref, E, what = _gemm_ref(d, ALPHA_RAND, **kw)
            note(what, f"bodies-{M}x{N}x{K}+{K2}-{form}", _gemm_twin(d, ALPHA_RAND, **kw), ref, E)
    for (M, N, K2) in [(1, 131, 64), (5, 40, 0), (5, 144, 64), (16, 131, 0), (16, 8, 64)]:
        d = _gemm_inputs(M, N, SKINNY_K, K2, "rand")
        for form in ("bias+res", "f32+bias+acc", "bias"):
            _, ref, E, what = _gemm_ref(d, ALPHA_RAND, c_epi=6, **FORMS[form])
            note(what, f"skinny-{M}x{N}+{K2}-{form}", _gemm_twin(d, ALPHA_RAND, **FORMS[form]), ref, E)
    d = _gemm_inputs(130, 131, 320, 0, "rand")
    c0 = _pattern(133, 144, F32)[1:131, 4:135]
    _, ref, E, what = _gemm_ref(d, ALPHA_RAND, f32=True, accumulate=True, c_epi=4, c0=c0)
    note(what, "splitk-320/3", _gemm_twin(d, ALPHA_RAND, f32=True, accumulate=True, c0=c0), ref, E)
    for rows in FP8_ROWS:
        for (M, N, K, res, f32, _) in _fp8_cases(rows, "rand"):
            d = _fp8_inputs(M, N, K, "rand")
            _, ref, E, what = _fp8_ref(d, bool(res), f32)
            note(what, f"fp8-{M}x{N}x{K}", _fp8_twin(d, bool(res), f32), ref, E)
    for (M, N, R, m_chunk) in WGRAD:
        y, t = _wgrad_inputs(M, N, R, "rand")
        al = _f32(ALPHA_RAND)
        ref, S = y.to(F64).T @ t.to(F64), y.to(F64).abs().T @ t.to(F64).abs()
        c0 = _pattern(N + 3, -(-(R + 5) // 8) * 8 + 4, F32)[1:1 + N, 4:4 + R].to(F64)
        E = (M + 2 + _n_chunks(M, N, m_chunk)) * U32 * (abs(al) * S + c0.abs())
        note("wgrad", f"wgrad-{M}x{N}x{R}", _wgrad_twin([y], t, R, c0, M, N, m_chunk), al * ref + c0, E)
    # the masks of the twin's LoRA cases: any fixed pattern of the right density serves (the kernels' own hash is project code)
    for (r, targets) in RANK_CASES:
        for (M, K) in LORA_SHAPES:
            x, A, dts = _lora_operands(r, targets, M, K, "rand")
            g = torch.Generator().manual_seed(r + targets)
            masks = [(torch.rand(M, K, generator=g) >= 0.25).to(F64) for _ in range(targets)]
            v, E = _lora_down_ref(x, A, masks, 0.25, ALPHA_RAND, r, targets)
            note("lora_down", f"r{r}x{targets}-{M}x{K}", _lora_down_twin(x, A, masks, 0.25, ALPHA_RAND, r, targets), v, E)
            v, E = _lora_up_ref(dts, A, masks, 0.25, r, targets)
            note("lora_up", f"r{r}x{targets}-{M}x{K}", _lora_up_twin(dts, A, masks, 0.25, r, targets), v, E)
        M, K = 70, 136
        x, A, dts = _lora_operands(r, targets, M, K, "rand")
        g = torch.Generator().manual_seed(r + targets)
        masks = [(torch.rand(M, K, generator=g) >= 0.25).to(F64) for _ in range(targets)]
        al = _f32(ALPHA_RAND)
        R = A.shape[0]
        ref, S = torch.zeros(K, R, dtype=F64), torch.zeros(K, R, dtype=F64)
        for j, x64 in enumerate(_masked64(x, masks, 0.25)):
            T = dts[:, j * r:(j + 1) * r].to(F64)
            ref[:, j * r:(j + 1) * r], S[:, j * r:(j + 1) * r] = x64.T @ T, x64.abs().T @ T.abs()
        c0 = _pattern(K + 3, -(-(R + 5) // 8) * 8 + 4, F32)[1:1 + K, 4:4 + R].to(F64)
        E = (M + 3 + _n_chunks(M, K, 32)) * U32 * (abs(al) * S + c0.abs()) + U * abs(al) * S
        note("wgrad_drop", f"wgrad-drop-r{r}x{targets}", _wgrad_twin(_masked_twin(x, masks, 0.25), dts, r, c0, M, K, 32), al * ref + c0, E)
    return worst, where


def _wgrad_twin(ys, t, rank, c0, M, N, m_chunk):
    """float32: per row chunk a sequential sum over its rows, times alpha, added to C one chunk after the other (the atomics' rounding
    points, in the chunks' order); ys: the operand per target (one entry: every column of t)"""
    R = t.shape[1]
    rows = _chunk_rows(M, N, m_chunk)
    c = c0.to(F32).clone()
    for m0 in range(0, M, rows):
        for j, yj in enumerate(ys):
            cols = slice(j * rank, (j + 1) * rank) if len(ys) > 1 else slice(0, R)
            part = _seq_matmul32(yj[m0:m0 + rows].T.contiguous(), t[m0:m0 + rows, cols].T.contiguous())
            c[:, cols] = c[:, cols] + part * torch.tensor(ALPHA_RAND, dtype=F32)
    return c


def test_twin_ratio_is_the_recorded_one():
    """MARGIN's origin, reproducible without a GPU and without project code"""
    worst, where = _twin_worst()
    print(f"\n[gemm-family] twin worst ratios { {k_: round(v_, 4) for k_, v_ in worst.items()} } at {where}")
    for k_ in TWIN_WORST:
        # (to the digits written: elementwise float32 torch on a CPU is the same everywhere)
        assert math.isfinite(worst[k_]) and abs(worst[k_] - TWIN_WORST[k_]) <= 0.01 * TWIN_WORST[k_] + 5e-5, (k_, worst[k_], where.get(k_))
        assert MARGIN[k_] == 2 * TWIN_WORST[k_]
