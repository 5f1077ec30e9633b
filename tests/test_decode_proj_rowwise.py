"""The weight-streaming projections of the token loop — k_decgemm.hip (bra_dec_gemm2, bra_dec_gemm2_packed, bra_dec_gemm2_fp8, bra_row_sumsq,
bra_dec_pack_weights_rows, bra_dec_pack_weights_fp8), the tile epilogue and statistics fold of bra_decgemm.h, and the first-generation
bra_dec_gemm of k_decfused.hip — element by element against float64 statements of the same operations, in the manner and with the
helpers of tests/test_gemm_family_rowwise.py (read its docstring first: value sets, E, MARGIN, the window in a patterned buffer).

tests/test_kernels.py, tests/test_fp8_rollout.py and tests/test_decode_rows32.py bound one Frobenius ratio per output tensor, check
ss_out through its row sum and show the 32-row form equal to the 16-row form.  One wave's last k-step of one tile dropped, the residual of
a workgroup's later tiles read at the wrong pitch, the diagonal mode's second K half taken from the wrong lane, one group of the statistics
fold lost, rows 16 .. 31 taking the rstd of rows 0 .. 15, the fp8 scale of the neighbouring column, a wrong gate / up partner lane, an
unmasked tile maximum: each moves a few elements and passes there.  Here every element is held.

  exact   (no norm) x and W integers |v| <= 4, the residual an integer <= 256.  With K <= 9728 every partial sum is below 16 * 9728 < 2^24:
          exact in fp32 in any wave order, through any LDS hand-off.  fp32 outputs equal the float64 product bit for bit, bf16 outputs
          rnd(acc) and rnd(rnd(acc) + res) (dg2_epilogue).  W is dense and random: every (tile, k-step, lane) fragment differs from every
          other one, a fragment read from the wrong place changes the sum.  Element (1, 3) is planted at 257 (x[1, :17] and W[3, :17] set,
          W[3, 17:] = 0) and sums beyond 256 land on ties by themselves; `ties` is asserted per group of cases.
          fp8: W integers in [-7, 7] with a 7 in every row: scale = 7 / 448 = 2^-6 (asserted), codes 64 W (asserted through
          test_fp8_rollout's unpack helper), partial sums <= 4 * 448 * 6144 < 2^24: exact as above.
          Tile maxima equal the maximum of the stored fp32 logits of the tile bit for bit (any value set).  ss_out[m, tile] is the sum of
          squares of the STORED bf16 values of the tile's columns: bit for bit wherever the float64 sum is below 2^24 (integers: every
          partial sum is then exact; decided per (row, tile), and the edge, later-tile and fp8 cases assert that some entries were held
          this way), otherwise — and on real values — within (columns + 2) * 2^-24 of the float64 sum.
  random  x, W ~ N(0, 0.5) bf16, residual N(0, 1), norm weight 1 + 0.1 N(0, 1), eps = 1e-6.  err <= MARGIN[what] * E, E first order:
              E = (K + 2) u S                 S = sum_k |xn_mk| |w_nk| (xn the normalised activation in float64; x where there is no norm)
                  + 2 U S      NORM 1: bf16(w * bf16(x * rstd)) before the MFMA, two rounding points on the activation
                  +   U S      NORM 2: bf16(W * w) once in the packer; rstd * acc in fp32 is one of the two epilogue roundings of (K + 2)
                  + tau_rstd u S   with a norm: rstd from the device's reciprocal square root — tests/test_layer_glue_rowwise.py's allowance
                               tau_rstd = (n_l + steps + 5) / 2 + 2 [u] (rsqrt itself an ulp = 2 u), here n_l = nss_in / 8 partials per
                               lane, steps = 3 butterfly steps (first generation, which sums x^2 itself: n_l = 8 ceil(K / 2048) squares per
                               thread, steps = 6 butterfly steps + 3 additions across the waves: _v1_tau)
                  + U |v|                     bf16 output;  residual form: U |rnd(v)| + U |out|
              fp8: the e4m3 rounding belongs to the packer — the reference multiplies the decoded codes the device produced by the
              device's scales; (K + 3): the scale is one more fp32 product.
          The statistics handed in are positive partials of this module's making whose sum is near sum x^2: the reference folds the
          fp32 numbers the kernel receives, in float64.
          MARGIN = 2 x TWIN_WORST; the twin is float32 torch with sequential accumulation and .to(bfloat16) at the points above, no
          project code; test_twin_ratio_is_the_recorded_one measures it again.  No margin was fitted to a kernel's output.
  SwiGLU  tests/test_layer_glue_rowwise.py's forward rule: bit for bit against the float64 twin bf16(bf16(silu(bf16 g)) * bf16 u), one
          bf16 ulp allowed only where silu(g) lies within tau_silu of a rounding boundary, at most 1 % of the elements.  Inputs as that
          module and the GEMM module choose them: x = +-2^j, gate rows four entries +-{1, 2, 4}, up rows one entry (u = +-2^k), norm
          weights powers of two: g is an exact fp32 number — g0 without norm, bf16(rstd) g0 under NORM 1 (no rstd within tau_rstd of a
          bf16 boundary: asserted), fp32(rstd g0) under NORM 2 (no g within (tau_rstd + 1) u of a bf16 boundary: asserted).
  probe   the statistics fold alone: folded form, fp32 output, x one-hot per row, W' entries +-2^j, ss_in a different positive number in
          every column and another set per row, rows >= M poisoned with 1e30: out[m, n] / W'[n, k_m] = rstd_m must be
          rsqrt(sum of ALL columns / K + eps) within tau_rstd u, at nss_in = 32, 64, 160, 256 and M = 5 .. 32 (which row, which columns,
          which of the eight groups, rs_lds[16 + ..] for rows 16 .. 31); NORM 1 through a one-hot W: out = w_k x_mk bf16(rstd_m).

The dispatch mirror (_mirror) restates, independently, what bra_decgemm.h states once (dg2_waves_and_chunks, dg2_diag, dg2_kernel_exists,
dg2_form_of):
    fast     packed, no in-register norm, K exactly one register round (waves x chunks k-steps): the FAST instantiation
    single   K exactly one round through the general kernel (row-major weights or NORM 1)
    clamped  one round with steps past K clamped and zeroed
    multi    the multi-round loop
A form is (rows class 8 / 16 / 32, tile mode, waves, chunks, kind, NORM, packed, epilogue).  _reachable() walks every K % 32 == 0 up to 9728
(the exact set's limit and the largest K of a supported model); FORM_CASES picks the smallest case of every form and
test_every_reachable_form_has_a_case proves the two sets equal; every form the launcher refuses is asserted refused
(test_refused_forms_are_refused, test_rows32_refusals_follow_the_exported_rule); test_exported_form_is_the_mirrors reads the launcher's
choice itself (bra_dec_gemm2_form, no launch) at every call of the walk.  dg2_waves_and_chunks never selects (16, 4) (16 waves have at
least 8 steps each) or, for the same reason, (8, 4): there are no such kernels (tests/test_isa.py holds the compiled set to the list).
<= 8 rows with a bf16 epilogue and K % 64 == 0 reach 16-column tiles only at N = 2064 (packed) or N % 8 != 0 (row-major, N = 44).

Emulator cases above 4.3e6 weight elements are skipped (`emulator: ...`); the mirror names a smaller case of the same form for each.
Worst device ratios go to dec_proj_rowwise_ratios.json in BRA_TEST_EVIDENCE_DIR (else test_evidence/).
"""
import collections
import ctypes
import functools
import json
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bioreason_amd import ops, _lib                                                          # noqa: E402
from test_gemm_family_rowwise import (_bf, _assert_bits, _ties, _ratio, _Window, _pattern, _randint, _seq_matmul32, _wide,   # noqa: E402
                                      U, U32)
from test_layer_glue_rowwise import _near, _ord, _tau_sg, _sigmoid64, NEAR_CAP                 # noqa: E402
from test_fp8_rollout import unpack_fp8_fast                                                 # noqa: E402

BF, F32, F64, F8 = torch.bfloat16, torch.float32, torch.float64, torch.float8_e4m3fn
EPS = 1e-6
UNSUPPORTED = _lib.BRA_ERR_UNSUPPORTED
K_MAX = 9728
EMU_MAX = 4.3e6
POISON = 1.0e30

# The rounding twin's worst err / E per quantity over RAND_CASES and V1_RAND (CPU) and the case that reached it.  n0 / n1 / n2: no norm,
# NORM 1, NORM 2; f8 / f8n2: fp8 weights without / with the folded norm.
TWIN_WORST = {
    "n0_f32": 0.01046,      # 8x48x96 row-major (the bound is the worst case of K aligned roundings; a sum's actual error grows like its root)
    "n0_bf16": 1.832,       # 8x40x96: one bf16 rounding, worst case 2 U
    "n0_res": 1.613,        # 5x40x96
    "n1_f32": 0.3026,       # 8x48x96: the two activation roundings carry the bound, 2 U S against a random sum of 96 of them
    "n1_bf16": 0.2871,      # first generation, 5x40x96
    "n1_res": 0.3818,       # 5x40x96
    "n2_f32": 0.3899,       # 8x48x96 packed
    "n2_bf16": 0.5045,      # 8x48x96 packed
    "n2_res": 0.7034,       # 5x48x96 packed
    "f8_f32": 0.001154,     # 8x48x512
    "f8_res": 1.142,        # 8x40x1024
    "f8n2_f32": 0.0009842,  # 8x48x512
    "f8n2_bf16": 1.355,     # 8x40x1024
}
MARGIN = {k_: 2 * v_ for k_, v_ in TWIN_WORST.items()}

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIO_FILE = os.path.join(os.environ.get("BRA_TEST_EVIDENCE_DIR") or os.path.join(ROOT, "test_evidence"), "dec_proj_rowwise_ratios.json")


# ----------------------------------------------------------------------------- the dispatch mirror
@functools.lru_cache(maxsize=None)
def _waves_chunks(nsteps, wide):
    """dg2_waves_and_chunks"""
    nw = 16 if (wide and nsteps >= 128) else (8 if nsteps >= 64 else 4)
    spw = -(-nsteps // nw)
    nl = 12 if (spw >= 12 and spw % 12 == 0) else (10 if (spw == 10 and nw == 8) else (8 if spw > 4 else 4))
    return nw, nl


def _diag(M, N, K, act, f32):
    """the 8-column (diagonal) tile rule: dg2_diag_tiles and what dec_gemm2_any adds"""
    return M <= 8 and not act and not f32 and K % 64 == 0 and N % 8 == 0 and (N + 15) // 16 < 256 and N // 8 <= 256


@functools.lru_cache(maxsize=None)
def _rows32_ok(K, normed, packed):
    """17 .. 32 rows: is there a kernel for this K?  (the library's answer: bra_dec_gemm2_rows32_ok)"""
    if K <= 0 or K % 32:
        return False
    nsteps = K // 32
    nw, nl = _waves_chunks(nsteps, True)
    if nsteps > nw * nl:
        return (not normed) and (nw < 16 or (nl == 8 and packed))
    if packed and nsteps == nw * nl and not (normed and nw == 16 and nl == 12):
        return True
    return nw * nl <= 64


Form = collections.namedtuple("Form", "rows mode nw nl kind norm packed epi")
EPIS = ("bf16", "res", "act", "f32", "f32max")


def _form_of(M, N, K, epi, norm, packed, fp8=False):
    """-> (form, refused, tiles, workgroups, rounds)"""
    act, f32 = epi == "act", epi in ("f32", "f32max")
    rows = 8 if M <= 8 else (16 if M <= 16 else 32)
    diag = _diag(M, N, K, act, f32)
    nsteps = K // (64 if diag else 32)
    nw, nl = _waves_chunks(nsteps, rows > 8)
    rounds = -(-nsteps // (nw * nl))
    NORM = 0 if not norm else (2 if packed & 2 else 1)
    ntiles = N // 8 if diag else -(-N // 16)
    gmax = ntiles if nw == 16 else (256 if nw >= 8 else 512)
    fast = NORM != 1 and bool(packed & 1) and nsteps == nw * nl
    kind = "multi" if rounds > 1 else ("fast" if fast else ("single" if nsteps == nw * nl else "clamped"))
    refused = (rows > 8 and NORM == 1) or (NORM == 2 and rounds != 1) or (rows == 32 and not _rows32_ok(K, NORM == 2, bool(packed & 1)))
    if fp8:
        # e4m3 images: packed, norm folded or absent, the fast form alone (an even number of chunks: two k-steps per request), in every
        # row class — 17 .. 32 rows where the bf16 rule above has the fast form too (not the folded norm on 16 waves x 12 chunks)
        refused = refused or not fast or nl % 2 == 1 or not (packed & 1) or (rows == 8 and nw == 16)
    return Form(rows, int(diag), nw, nl, kind, NORM, packed, epi), refused, ntiles, min(ntiles, gmax), rounds


def _mirror(M, N, K, epi="bf16", norm=False, packed=0, fp8=False):
    """what dec_gemm2_any / launch_dg2 do with this call -> dict(form, refused, ntiles, grid, later, rounds)"""
    form, refused, ntiles, grid, rounds = _form_of(M, N, K, epi, norm, packed, fp8)
    # tiles past the grid are the only ones whose residual is loaded in the epilogue (dg2_epilogue: !have_res)
    return {"form": form, "refused": refused, "ntiles": ntiles, "grid": grid, "later": ntiles > grid, "rounds": rounds}


NORM_PACKED = [(False, 0), (False, 1), (True, 0), (True, 1), (True, 3)]          # (norm weight given, `packed`); above 8 rows NORM 1 is refused
M_OF = {8: (1, 5, 8), 16: (9, 12, 16), 32: (17, 24, 31, 32)}
# K walked first: the shapes named for each form (512 .. 3072: the six single-round forms on 32-deep steps, 1024 .. 6144 on 64-deep steps,
# 96 / 320 one clamped round, 3328 / 9728 multi-round, 4096 / 6144 the 16-wave forms), then every other multiple of 32 in rising order
K_FIRST = [512, 1024, 1536, 2048, 2560, 3072, 96, 320, 3328, 4096, 5120, 6144, 9728]


def _shape_candidates(rows, epi, packed):
    """N small; <= 8 rows with a bf16 epilogue leave the diagonal mode through K % 64 = 32, N % 8 != 0 (row-major only) or N = 2064"""
    if epi == "act":
        return (48,)
    if epi in ("f32", "f32max") or rows > 8:
        return (48,) if packed else (40,)
    return (40, 48, 2064) if packed else (40, 44)


@functools.lru_cache(maxsize=None)
def _reachable():
    """-> (form -> the (M, N, K) chosen for it, refused form -> (M, N, K)): among the shapes that take a form, one the emulator runs before
    one it skips, a K the decode work names (K_FIRST) before another, then the fewest weight elements"""
    ok, no = {}, {}
    for rows in (8, 16, 32):
        for (norm, packed) in NORM_PACKED:
            for epi in EPIS:
                for K in range(32, K_MAX + 1, 32):
                    for N in _shape_candidates(rows, epi, packed):
                        f, refused = _form_of(M_OF[rows][0], N, K, epi, norm, packed)[:2]
                        if packed and N % (8 if f.mode else 16):
                            continue                                  # (no packed image of a ragged tile: BRA_ERR_ARG, not a form)
                        cost = (N * K > EMU_MAX, K not in K_FIRST, N * K)
                        tgt = no if refused else ok
                        if f not in tgt or cost < tgt[f][0]:
                            tgt[f] = (cost, N, K)
    out = []
    for tgt in (ok, no):
        out.append({f: (M_OF[f.rows][j % len(M_OF[f.rows])], N, K) for j, (f, (_, N, K)) in enumerate(sorted(tgt.items()))})
    return out[0], out[1]


Case = collections.namedtuple("Case", "M N K epi norm packed vals nss layout strided")


def _case_of(form, shape, j=0):
    M, N, K = shape
    return Case(M, N, K, form.epi, form.norm != 0, form.packed, "exact" if form.norm == 0 else "rand", (32, 64, 160, 256)[j % 4],
                ("lds", "direct")[j % 2], j % 3 == 1)


@functools.lru_cache(maxsize=None)
def _form_cases():
    ok, _ = _reachable()
    return {f: _case_of(f, shape, j) for j, (f, shape) in enumerate(sorted(ok.items()))}


def _groups():
    """the form cases by (rows class, tile mode, waves, chunks, kind): one pytest case each"""
    g = collections.defaultdict(list)
    for f, c in _form_cases().items():
        g[(f.rows, f.mode, f.nw, f.nl, f.kind)].append(c)
    return dict(sorted(g.items()))


# ----------------------------------------------------------------------------- inputs
def _pow2(g, shape, lo, hi):
    return (2.0 ** torch.randint(lo, hi + 1, shape, generator=g).to(F64)) * (torch.randint(0, 2, shape, generator=g).to(F64) * 2 - 1)


@functools.lru_cache(maxsize=64)
def _inputs(M, N, K, vals, attempt=0):
    """bf16 operands on the CPU.  exact: integers with the planted 257; rand: N(0, 0.5); act: the SwiGLU set (N = 16 tiles of [8 gate | 8 up])"""
    g = torch.Generator().manual_seed(100003 * M + 1009 * N + 7 * K + {"exact": 0, "rand": 1, "act": 2}[vals] + 3 * attempt)
    if vals == "exact":
        assert K <= K_MAX
        x, W, res = _randint(g, (M, K), 4), _randint(g, (N, K), 4), _randint(g, (M, N), 256)
        if M > 1 and N > 3:
            x[1, :16], W[3, :16], x[1, 16], W[3, 16], W[3, 17:] = 4, 4, 1, 1, 0
        nw = torch.ones(K, dtype=F64)
    elif vals == "rand":
        x, W = torch.randn(M, K, generator=g, dtype=F64) * 0.5, torch.randn(N, K, generator=g, dtype=F64) * 0.5
        res, nw = torch.randn(M, N, generator=g, dtype=F64), 1 + 0.1 * torch.randn(K, generator=g, dtype=F64)
    else:
        assert N % 16 == 0
        x = _pow2(g, (M, K), -2, 0)
        W = torch.zeros(N, K, dtype=F64)
        rows = torch.arange(N)
        gate = (rows % 16) < 8
        for i in range(4):
            c = torch.randint(0, K, (N,), generator=g)
            v = _pow2(g, (N,), 0, 2)
            put = gate if i else torch.ones(N, dtype=torch.bool)       # up rows: one entry
            W[rows[put], c[put]] = v[put]
        res, nw = torch.zeros(M, N, dtype=F64), _pow2(g, (K,), -1, 1).abs()
    d = {"M": M, "N": N, "K": K, "vals": vals}
    for k_, v_ in (("x", x), ("W", W), ("res", res), ("nw", nw)):
        d[k_] = v_.to(BF)
    if vals == "exact":
        acc = d["x"].to(F64) @ d["W"].to(F64).T
        assert (M == 1 or N <= 3 or acc[1, 3] == 257) and (d["x"].to(F64).abs() @ d["W"].to(F64).abs().T).max() < 2 ** 24
    return d


def _stats(d, nss, M_rows):
    """ss_in [M_rows, nss] fp32: positive partials, different in every column and row, summing to about sum x^2 of the row (rows >= M:
    POISON) -> (tensor, rstd in float64 from the fp32 numbers themselves)"""
    M, K = d["M"], d["K"]
    g = torch.Generator().manual_seed(nss + 31 * M + K)
    w = torch.rand(M, nss, generator=g, dtype=F64) + 0.25
    tot = (d["x"].to(F64) ** 2).sum(1, keepdim=True).clamp_min(1.0)
    ss = torch.full((M_rows, nss), POISON, dtype=F32)
    part = w / w.sum(1, keepdim=True) * tot
    for _ in range(8):          # (no row's rstd within 64 u of a bf16 boundary: the SwiGLU cases under NORM 1 need bf16(x * rstd) decided)
        ss[:M] = part.to(F32)
        rstd = torch.rsqrt(ss[:M].to(F64).sum(1) / K + float(torch.tensor(EPS, dtype=F32)))
        near = _near(rstd, 64 * U32 * rstd)
        if not near.any():
            break
        part = torch.where(near[:, None], part * 1.003, part)
    assert not near.any()
    return ss, rstd


def _tau_rstd(nss):
    """tests/test_layer_glue_rowwise.py: tau_rstd = (n_l + steps + 5) / 2 + 2 [u]; a lane folds nss / 8 partials, then 3 butterfly steps"""
    return (nss // 8 + 3 + 5) / 2 + 2


def _stat_rows(M):
    return 8 if M <= 8 else (16 if M <= 16 else 32)


# ----------------------------------------------------------------------------- references
def _swiglu_pairs(v):
    """[M, N] columns in tiles of [8 gate | 8 up] -> (g, u) [M, N / 2]"""
    t = v.view(v.shape[0], v.shape[1] // 16, 2, 8)
    return t[:, :, 0].reshape(v.shape[0], -1), t[:, :, 1].reshape(v.shape[0], -1)


def _bound_ref(xn, Wf, K, what, res, c_epi=2, act_round=0, tau=0.0):
    """xn [M, K] (normalised activations, float64), Wf [N, K] float64 -> (ref, E) per the module docstring; act_round: bf16 rounding points
    on the operands (NORM 1: 2, NORM 2: 1)"""
    v, S = xn @ Wf.T, xn.abs() @ Wf.abs().T
    E = ((K + c_epi) * U32 + act_round * U + tau * U32) * S
    if what == "f32":
        return v, E
    if what == "bf16":
        return v, E + U * v.abs()
    out = _bf(v) + res
    return v + res, E + U * _bf(v).abs() + U * out.abs()


def _what(epi):
    return {"bf16": "bf16", "res": "res", "f32": "f32", "f32max": "f32"}[epi]


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
    if not ratios:
        return
    print(f"\n[dec-proj] {name}: " + " ".join(f"{k_} {v_:.3f}" for k_, v_ in ratios.items()))
    _record(name, ratios, dev)
    for k_, v_ in ratios.items():
        assert v_ <= MARGIN[k_], (name, k_, v_, MARGIN[k_])


class _WindowAt(_Window):
    """_Window with the column offset and the pitch given"""

    def __init__(self, M, N, dtype, dev, off, ld):
        self.M, self.N, self.off = M, N, off
        buf = _pattern(M + 3, ld, dtype)
        self.buf = buf.to(dev)
        self.before = buf.clone()
        self.win = self.buf[1:1 + M, off:off + N]


def _swiglu_twin(d, norm, rstd=None, tau_rstd=0.0):
    """the float64 twin of the SwiGLU epilogue on the exact gate / up values -> (want bf16, near, undecided, ulps allowed where near).
    Without norm u = +-2^k: bf16(silu) * u is exact and an inner flip of silu is one output ulp.  Under a norm u = bf16(rstd 2^k) is no power of
    two: the product is a real one and an inner flip may cost two output ulps (tests/test_layer_glue_rowwise.py, _swiglu_inputs, measured
    there).  NORM 1: bf16(w bf16(x rstd)) = w x bf16(rstd) for powers of two, g = bf16(rstd) g0 an exact fp32 number.  NORM 2: g = fp32(rstd g0),
    within (tau_rstd + 1) u of the float64 product: where THAT is within reach of a bf16 boundary the element is `undecided` (not held)"""
    X, W64, nwf = d["x"].to(F64), d["W"].to(F64), d["nw"].to(F64)
    if norm == 0:
        g64, uu = _swiglu_pairs(X @ W64.T)
        assert torch.equal(torch.log2(uu.abs()), torch.log2(uu.abs()).round())
        undecided, ulps = torch.zeros_like(g64, dtype=torch.bool), 1
    elif norm == 1:
        assert not _near(rstd, tau_rstd * U32 * rstd).any()
        g0, u0 = _swiglu_pairs((X * nwf) @ W64.T)
        g64, uu = _bf(rstd)[:, None] * g0, _bf(rstd)[:, None] * u0
        undecided, ulps = torch.zeros_like(g64, dtype=torch.bool), 2
    else:
        tau = (tau_rstd + 1) * U32
        g0, u0 = _swiglu_pairs(X @ (W64 * nwf).T)
        g64, uu = rstd[:, None] * g0, rstd[:, None] * u0
        undecided, ulps = _near(g64, tau * g64.abs()) | _near(uu, tau * uu.abs()), 2
    gb, ub = _bf(g64), _bf(uu)
    assert (gb.abs() <= 64).all() and (ub != 0).all()
    silu = gb * _sigmoid64(gb)
    near = _near(silu, U32 * _tau_sg(gb) * silu.abs())
    return (_bf(silu) * ub).to(BF), near, undecided, ulps


def _swiglu_case(M, N, K, norm, nss):
    """the first of eight input sets whose twin ALONE stays within the cap (decided on the CPU, before any kernel runs)"""
    for attempt in range(8):
        d = _inputs(M, N, K, "act", attempt)
        ss, rstd = _stats(d, nss, _stat_rows(M)) if norm else (None, None)
        want, near, undecided, ulps = _swiglu_twin(d, norm, rstd, _tau_rstd(nss))
        if (near | undecided).float().mean().item() <= NEAR_CAP:
            return d, ss, rstd, (want, near, undecided, ulps)
    raise AssertionError(("no SwiGLU input set within the cap", M, N, K, norm, nss))


def _assert_swiglu(name, got, twin):
    """the forward rule of tests/test_layer_glue_rowwise.py: bit for bit, `ulps` allowed only where silu(g) is boundary-near"""
    want, near, undecided, ulps = twin
    assert (near | undecided).float().mean().item() <= NEAR_CAP, name
    dlt = (_ord(got.detach().cpu()) - _ord(want)).abs()
    ok = (dlt == 0) | (near & (dlt <= ulps)) | undecided
    assert bool(ok.all()), (name, int((~ok).sum()), torch.nonzero(~ok)[:8].tolist())


# ----------------------------------------------------------------------------- one call of bra_dec_gemm2 / _packed, every output held
def _check_ss(name, ss_got, stored, ncol, ntiles):
    """ss_out [M, ntiles] against the stored bf16 outputs: bit for bit where the float64 sum of integer squares is below 2^24, else within
    (columns + 2) 2^-24 -> how many were held bit for bit"""
    M, N = stored.shape
    pad = torch.zeros(M, ntiles * ncol, dtype=F64)
    pad[:, :N] = stored.to(F64) ** 2
    want = pad.view(M, ntiles, ncol).sum(-1)
    got = ss_got.to(F64)
    integral = torch.equal(stored.to(F64), stored.to(F64).round())
    exact = (want < 2 ** 24) if integral else torch.zeros_like(want, dtype=torch.bool)
    bad = (exact & (got != want)) | (~exact & ((got - want).abs() > (ncol + 2) * U32 * want))
    assert not bad.any(), f"{name}: ss_out differs in {int(bad.sum())} of {bad.numel()} (row, tile) entries, first {torch.nonzero(bad)[0].tolist()}: " \
                          f"got {got[tuple(torch.nonzero(bad)[0])].item()} want {want[tuple(torch.nonzero(bad)[0])].item()}"
    return int(exact.sum())


def _run(dev, c, ratios, tally, name=None):
    """the call of Case c into sentinel windows; asserts every output element, the statistics / tile maxima and everything around them"""
    M, N, K, epi = c.M, c.N, c.K, c.epi
    act, f32 = epi == "act", epi in ("f32", "f32max")
    m = _mirror(M, N, K, epi, c.norm, c.packed)
    f = m["form"]
    assert not m["refused"], (c, f)
    name = name or f"{f.rows}r-m{f.mode}-{f.nw}x{f.nl}-{f.kind}-n{f.norm}-p{f.packed}-{epi}-{M}x{N}x{K}"
    nss = c.nss if c.norm else 0
    if act:
        d, ss_cpu, rstd, twin = _swiglu_case(M, N, K, f.norm, nss)
    else:
        d = _inputs(M, N, K, c.vals)
        ss_cpu, rstd = _stats(d, nss, _stat_rows(M)) if c.norm else (None, None)
    lib = _lib.get_lib()
    x = _wide(d["x"], dev) if c.strided else d["x"].to(dev)
    Wd, nwd = d["W"].to(dev), (d["nw"].to(dev) if c.norm else None)
    if c.packed:
        Wk = ops.dec_pack_weights(Wd, act=act, out_f32=f32, norm_w=nwd if c.packed == 3 else None, rows=8 if M <= 8 else 16)
        assert Wk is not None, name
        ldw = K
    else:
        Wk = _wide(d["W"], dev) if c.strided else Wd
        ldw = Wk.stride(0)
    ss_in = ss_cpu.to(dev) if c.norm else None
    No = N // 2 if act else N
    if f32 and c.strided:
        win = _WindowAt(M, No, F32, dev, 3, No + 9 + ((No + 9) % 4 == 0))     # an fp32 pitch that is no multiple of 4: the scalar store path
        assert win.win.stride(0) % 4
    else:
        win = _Window(M, No, F32 if f32 else BF, dev, c.layout)
    res = None
    if epi == "res":
        rw = _WindowAt(M, N, BF, dev, 4, N + 4 + (-(N + 4)) % 8 + 4) if (c.strided or N % 4) else None       # ldres = 4 mod 8 (the entry point wants ldres % 4 == 0)
        if rw is not None:
            rw.buf[1:1 + M, 4:4 + N] = d["res"].to(dev)
            res = rw.win
            assert res.stride(0) % 8 == 4
        else:
            res = d["res"].to(dev)
    ncol = 8 if f.mode else 16
    sw = _Window(M, m["ntiles"], F32, dev, "direct") if epi in ("res", "f32max") else None
    args = [x, x.stride(0), ss_in, nss, nwd, EPS, Wk, ldw, res, res.stride(0) if res is not None else 0, win.win, win.win.stride(0),
            sw.win if sw else None, sw.win.stride(0) if sw else 0, M, N, K, int(act), int(f32)]
    if c.packed:
        rc = lib.call_rc("bra_dec_gemm2_packed", *args, c.packed, _lib.current_stream(x))
    else:
        rc = lib.call_rc("bra_dec_gemm2", *args, _lib.current_stream(x))
    assert rc == 0, (name, rc)
    got = win.result(name)
    assert not torch.isnan(got.float()).any(), name
    # ---- the reference
    X, W64, R = d["x"].to(F64), d["W"].to(F64), d["res"].to(F64)
    if act:
        _assert_swiglu(name, got, twin)
        tally["act"] = tally.get("act", 0) + 1
        return got
    if f.norm == 0 and c.vals == "exact":
        acc = X @ W64.T
        if f32:
            want = acc.to(F32)
        elif epi == "res":
            want = (_bf(acc) + R).to(BF)
            tally["ties"] = tally.get("ties", 0) + _ties(acc) + _ties(_bf(acc) + R)
        else:
            want = acc.to(BF)
            tally["ties"] = tally.get("ties", 0) + _ties(acc)
        _assert_bits(name, got, want)
    else:
        if f.norm:
            xn = X * rstd[:, None] * d["nw"].to(F64)
            ref, E = _bound_ref(xn, W64, K, _what(epi), R, act_round=2 if f.norm == 1 else 1, tau=_tau_rstd(nss))
        else:
            ref, E = _bound_ref(X, W64, K, _what(epi), R)
        key = f"n{f.norm}_{_what(epi)}"
        ratios[key] = max(ratios.get(key, 0.0), _ratio((got.to(F64) - ref).abs(), E))
    # ---- statistics / tile maxima: windows of their own, functions of the STORED outputs
    if epi == "res":
        tally["ss_exact"] = tally.get("ss_exact", 0) + _check_ss(name, sw.result(name + " ss_out"), got, ncol, m["ntiles"])
    if epi == "f32max":
        pad = torch.full((M, m["ntiles"] * 16), -math.inf, dtype=F32)
        pad[:, :N] = got
        _assert_bits(name + " tile maxima", sw.result(name + " tile maxima"), pad.view(M, m["ntiles"], 16).amax(-1))
    return got


def _emu_skip(dev, N, K, smaller):
    if dev.type == "cpu" and N * K > EMU_MAX:
        pytest.skip(f"emulator: {N} x {K} weights; the same form at {smaller}")


# ----------------------------------------------------------------------------- 1: the table
def test_every_reachable_form_has_a_case():
    """every (rows, mode, waves, chunks, kind, NORM, packed, epilogue) the launcher can take for K <= 9728 has a case here, the cases take
    the forms written next to them, and the (waves, chunks) pairs are the ones dg2_waves_and_chunks can return"""
    ok, no = _reachable()
    cases = _form_cases()
    assert set(cases) == set(ok) and len(ok) > 300
    for f, c in cases.items():
        m = _mirror(c.M, c.N, c.K, c.epi, c.norm, c.packed)
        assert m["form"] == f and not m["refused"], (f, c)
    pairs = {(f.nw, f.nl) for f in ok}
    assert pairs == {(4, 4), (4, 8), (4, 12), (8, 8), (8, 10), (8, 12), (16, 8), (16, 12)}          # never (16, 4), never (8, 4)
    assert {f.kind for f in ok} == {"fast", "single", "clamped", "multi"}
    assert {(f.rows, f.mode) for f in ok} == {(8, 0), (8, 1), (16, 0), (32, 0)}
    # the shapes the decode work names
    for (M, N, K, epi, norm, packed), (mode, nw, nl, kind) in {
            (8, 48, 512, "f32", False, 1): (0, 4, 4, "fast"), (8, 48, 3072, "act", True, 3): (0, 8, 12, "fast"), (8, 48, 96, "f32", False, 0): (0, 4, 4, "clamped"),
            (8, 48, 3328, "f32", False, 1): (0, 8, 8, "multi"), (8, 48, 9728, "f32", False, 0): (0, 8, 8, "multi"), (8, 40, 6144, "res", False, 1): (1, 8, 12, "fast"),
            (8, 40, 320, "bf16", False, 0): (1, 4, 4, "clamped"), (8, 2048, 9728, "res", False, 1): (1, 8, 8, "multi"), (8, 2064, 2048, "res", False, 1): (0, 8, 8, "fast"),
            (16, 48, 4096, "res", False, 1): (0, 16, 8, "fast"), (16, 48, 6144, "res", False, 1): (0, 16, 12, "fast"), (12, 48, 9728, "res", False, 0): (0, 16, 8, "multi"),
            (32, 48, 6144, "bf16", False, 1): (0, 16, 12, "fast")}.items():
        f = _mirror(M, N, K, epi, norm, packed)["form"]
        assert (f.mode, f.nw, f.nl, f.kind) == (mode, nw, nl, kind), (M, N, K, f)
    assert _mirror(8, 2048, 2048)["form"].mode == 1 and _mirror(8, 2056, 2048)["form"].mode == 0       # N = 2048: the largest diagonal N
    assert _mirror(16, 48, 6144, "res", False, 1)["grid"] == 3                                          # (16, 12): one tile per workgroup
    # later tiles of a workgroup: the in-epilogue residual load runs there and nowhere else
    assert _mirror(8, 8208, 512, "res", False, 1)["later"] and _mirror(8, 8208, 512, "res", False, 1)["grid"] == 512
    assert _mirror(8, 4112, 2048, "res", False, 1)["later"] and _mirror(8, 4112, 2048, "res", False, 1)["grid"] == 256
    assert not any(_mirror(c.M, c.N, c.K, c.epi, c.norm, c.packed)["later"] for c in cases.values())


GROUPS = _groups()


@pytest.mark.parametrize("key", list(GROUPS), ids=lambda k_: f"{k_[0]}r-m{k_[1]}-{k_[2]}x{k_[3]}-{k_[4]}")
def test_forms_rowwise(backend, key):
    """every form of one (rows class, tile mode, waves, chunks, kind): all its NORM / packed / epilogue combinations, exact where there is
    no norm, under the bound with one; windows, strides and statistics widths rotate over the cases"""
    ratios, tally = {}, {}
    ran = 0
    for c in GROUPS[key]:
        if backend.type == "cpu" and c.N * c.K > EMU_MAX:
            continue                                                    # (N = 2064: the same (waves, chunks, kind) runs at N = 48 with fp32 output)
        _run(backend, c, ratios, tally)
        ran += 1
    assert ran > 0
    big = [c for c in GROUPS[key] if c.vals == "exact" and c.epi in ("bf16", "res") and (c.K >= 512 or c.epi == "res") and c.N * c.K <= EMU_MAX]
    assert not big or tally.get("ties", 0) > 0, f"no sum landed on a bf16 tie: {tally}"
    _assert_ratios("forms-" + "-".join(str(k_) for k_ in key), ratios, backend)


def test_refused_forms_are_refused(backend):
    """every form the mirror calls refused returns BRA_ERR_UNSUPPORTED and writes nothing"""
    _, no = _reachable()
    assert len(no) > 50
    lib = _lib.get_lib()
    for f, (M, N, K) in sorted(no.items()):
        act, f32 = f.epi == "act", f.epi in ("f32", "f32max")
        x, W, nw = (torch.ones(s_, dtype=BF, device=backend) for s_ in ((M, K), (N, K), (K,)))
        ss = torch.ones((_stat_rows(M), 32), dtype=F32, device=backend)
        win = _Window(M, N // 2 if act else N, F32 if f32 else BF, backend)
        rc = lib.call_rc("bra_dec_gemm2_packed", x, K, ss if f.norm else None, 32 if f.norm else 0, nw if f.norm else None, EPS, W, K, None, 0,
                         win.win, win.win.stride(0), None, 0, M, N, K, int(act), int(f32), f.packed, _lib.current_stream(x))
        assert rc == UNSUPPORTED, (f, M, N, K, rc)
        win.result(str(f))


def test_rows32_refusals_follow_the_exported_rule(backend):
    """17 .. 32 rows at every K of the module: BRA_ERR_UNSUPPORTED exactly where bra_dec_gemm2_rows32_ok says 0, and the mirror agrees with
    the export on every K up to 9728"""
    lib = _lib.get_lib()
    for K in range(32, K_MAX + 1, 32):
        for normed, packed in ((0, 0), (0, 1), (1, 1)):
            assert int(lib._dll.bra_dec_gemm2_rows32_ok(K, normed, packed)) == int(_rows32_ok(K, bool(normed), bool(packed))), (K, normed, packed)


ROWS32_K = [96, 320, 512, 1024, 1536, 2048, 2560, 3072, 3328, 4096, 6144, 9728]


@pytest.mark.parametrize("K", ROWS32_K)
def test_rows32_every_k(backend, K):
    """17 .. 32 rows at every K the forms name, row-major, packed and packed with the folded norm: BRA_ERR_UNSUPPORTED exactly where
    bra_dec_gemm2_rows32_ok says 0, and where it says 1 every element is held (not only equal to the 16-row call)"""
    lib = _lib.get_lib()
    ratios, tally = {}, {}
    for j, (norm, packed) in enumerate(((False, 0), (False, 1), (True, 3))):
        ok = int(lib._dll.bra_dec_gemm2_rows32_ok(K, int(norm), packed & 1))
        M = (17, 24, 31, 32)[(j + K // 32) % 4]
        epi = ("res", "f32max", "bf16")[(j + K // 64) % 3]
        assert _mirror(M, 48, K, epi, norm, packed)["refused"] == (not ok)
        if ok:
            _run(backend, Case(M, 48, K, epi, norm, packed, "rand" if norm else "exact", 64, "lds", bool(j % 2)), ratios, tally)
            continue
        x, W, nw = (torch.ones(s_, dtype=BF, device=backend) for s_ in ((M, K), (48, K), (K,)))
        ss = torch.ones((32, 64), dtype=F32, device=backend)
        win = _Window(M, 48, BF, backend)
        rc = lib.call_rc("bra_dec_gemm2_packed", x, K, ss if norm else None, 64 if norm else 0, nw if norm else None, EPS, W, K, None, 0,
                         win.win, win.win.stride(0), None, 0, M, 48, K, 0, 0, packed, _lib.current_stream(x))
        assert rc == UNSUPPORTED, (K, norm, packed, rc)
        win.result(f"rows32-{K}")
    _assert_ratios(f"rows32-{K}", ratios, backend)


def _exported_form(lib, M, N, K, epi, norm, packed, fp8=False, ldx=None, probed=0):
    """bra_dec_gemm2_form (debug ABI; launches nothing) -> dec_gemm2_kernel's ten template arguments, or the refusal code"""
    form = (ctypes.c_int * 10)()
    rc = int(lib._dll.bra_dec_gemm2_form(M, N, K, int(epi == "act"), int(epi in ("f32", "f32max")), int(norm), packed, int(fp8), ldx or K,
                                         N if epi == "res" else 0, 32 if norm else 0, probed, ctypes.addressof(form)))
    return rc if rc else tuple(form)


def _form_walk():
    """every call of _reachable()'s walk (the row count rotating over the class), then the e4m3 calls of the three row classes"""
    for rows in (8, 16, 32):
        for (norm, packed) in NORM_PACKED:
            for fp8 in ((False, True) if packed & 1 and (packed & 2 or not norm) else (False,)):
                for epi in EPIS:
                    for K in range(32, K_MAX + 1, 32):
                        for N in _shape_candidates(rows, epi, packed):
                            M = M_OF[rows][(K // 32) % len(M_OF[rows])]
                            if not (packed and N % (8 if _diag(M, N, K, epi == "act", epi in ("f32", "f32max")) else 16)):
                                yield M, N, K, epi, norm, packed, fp8


def test_exported_form_is_the_mirrors(debug_backend):
    """the launcher's own choice, read through bra_dec_gemm2_form without a launch, equals the mirror's at every call of the walk: row class,
    tile mode, waves, chunks, kind, NORM, packed, fp8, and refusal"""
    lib = _lib.get_lib()
    seen = set()
    for (M, N, K, epi, norm, packed, fp8) in _form_walk():
        f, refused = _form_of(M, N, K, epi, norm, packed, fp8)[:2]
        got = _exported_form(lib, M, N, K, epi, norm, packed, fp8)
        assert (got == UNSUPPORTED) == refused, (M, N, K, epi, norm, packed, fp8, got)
        if refused:
            continue
        mode, NORM, act, f32, nw, nl, wide, pk, fast, f8 = got
        nsteps = K // (64 if mode else 32)
        kind = "fast" if fast else ("multi" if nsteps > nw * nl else ("single" if nsteps == nw * nl else "clamped"))
        assert ({0: 8, 1: 16, 2: 32, 3: 32}[wide], mode, nw, nl, kind, NORM, pk, f8) == (f.rows, f.mode, f.nw, f.nl, f.kind, f.norm, packed & 1, int(fp8)), \
            (M, N, K, epi, norm, packed, fp8, got)
        assert (act, f32) == (int(epi == "act"), int(epi in ("f32", "f32max"))) and (wide == 3) == (f.rows == 32 and kind == "multi")
        seen.add(got)
    assert len(seen) > 400
    # outside the walk's strides: a probed call and one whose row pitch does not fit 24 bits leave the fast form for the general kernel,
    # which 32 rows have in the (waves, chunks) of at most 64 steps only
    assert _exported_form(lib, 8, 48, 512, "f32", False, 1)[6:] == (0, 1, 1, 0)
    assert _exported_form(lib, 8, 48, 512, "f32", False, 1, probed=1)[6:] == (0, 1, 0, 0)
    assert _exported_form(lib, 8, 48, 512, "f32", False, 1, ldx=1 << 24)[6:] == (0, 1, 0, 0)
    assert _exported_form(lib, 32, 48, 2048, "f32", True, 3, ldx=1 << 24)[4:] == (8, 8, 2, 1, 0, 0)
    assert _exported_form(lib, 32, 48, 2560, "f32", True, 3, ldx=1 << 24) == UNSUPPORTED
    assert _exported_form(lib, 8, 48, 512, "f32", False, 1, fp8=True, ldx=1 << 24) == UNSUPPORTED


# ----------------------------------------------------------------------------- 2: shapes the forms' smallest cases do not reach
# ragged and strided: row-major N = 40 (ragged last 16-column tile), 4104 (ragged last tile, 8 columns), 4107 (scalar store tail),
# windows with ldx > K, ldo > N, ldres = 4 mod 8, an odd fp32 pitch; diagonal N = 8, 40, 2048; M over every row count
EDGE = [Case(M, N, K, epi, False, packed, "exact", 32, layout, strided)
        for (M, N, K, epi, packed, layout, strided) in [
            (5, 40, 96, "res", 0, "direct", True), (8, 40, 96, "f32max", 0, "lds", True), (1, 40, 96, "bf16", 0, "lds", False),
            (8, 4104, 96, "res", 0, "lds", True), (5, 4107, 96, "res", 0, "lds", False), (8, 4107, 96, "f32max", 0, "direct", True),
            (8, 4107, 96, "bf16", 0, "direct", False), (12, 4107, 96, "res", 0, "lds", True), (24, 4107, 96, "f32max", 0, "lds", False),
            (31, 40, 512, "res", 0, "direct", True), (17, 4104, 96, "res", 0, "lds", False),
            (8, 8, 1024, "res", 1, "lds", False), (1, 8, 1024, "bf16", 0, "direct", False), (5, 40, 1024, "res", 1, "direct", True),
            (8, 2048, 1024, "res", 1, "lds", False), (5, 2048, 320, "res", 0, "direct", True),
            (9, 48, 512, "res", 1, "direct", True), (16, 48, 2048, "f32max", 1, "lds", True), (32, 48, 2048, "f32max", 1, "lds", True),
            (24, 48, 512, "res", 0, "direct", True), (31, 48, 9728, "res", 1, "lds", False), (12, 48, 9728, "res", 0, "lds", True)]]


@pytest.mark.parametrize("c", EDGE, ids=lambda c: f"{c.M}x{c.N}x{c.K}-{c.epi}-p{c.packed}" + ("-strided" if c.strided else ""))
def test_edges_exact(backend, c):
    """ragged last tiles, the scalar store tail, strided operands and outputs, the diagonal mode at its smallest and largest N, every row
    count: bit for bit; rows >= M, columns >= N and statistics columns >= the tile count still hold the pattern"""
    tally = {}
    _run(backend, c, {}, tally)
    if c.epi == "res":
        assert tally["ss_exact"] > 0


LATER = [(8, 8208, 512, 512), (5, 4112, 2048, 256), (16, 4112, 2048, 256), (24, 4112, 2048, 256)]


@pytest.mark.parametrize("M,N,K,cap", LATER)
def test_later_tiles_of_a_workgroup(backend, M, N, K, cap):
    """more tiles than the grid cap: the only shapes where a workgroup finishes a second (and third) tile — weights ping-pong, the epilogue
    wave rotates, and the residual is loaded in the epilogue (dg2_epilogue: !have_res) at its own pitch (ldres != ldo != N here)"""
    _emu_skip(backend, N, K, "none: the 256-workgroup cap needs K >= 2048; N = 8208 at K = 512 runs the 512 cap")
    m = _mirror(M, N, K, "res", False, 1)
    assert m["later"] and m["grid"] == cap and m["form"].kind == "fast"
    tally = {}
    for packed in (1, 0):
        _run(backend, Case(M, N, K, "res", False, packed, "exact", 32, "lds", True), {}, tally)
    assert tally["ties"] > 0 and tally["ss_exact"] > 0


# ----------------------------------------------------------------------------- 3: the random set
RAND_CASES = [Case(M, N, K, epi, norm, packed, "rand", nss, "lds", False)
              for (M, N, K, epi, norm, packed, nss) in [
                  (8, 48, 96, "f32", False, 0, 32), (8, 40, 96, "bf16", False, 0, 32), (5, 40, 96, "res", False, 0, 32),
                  (8, 48, 2048, "f32", False, 1, 32), (8, 40, 2048, "res", False, 1, 32), (5, 40, 6144, "bf16", False, 1, 32),
                  (12, 48, 2048, "res", False, 1, 32), (24, 48, 3328, "f32", False, 1, 32), (31, 48, 2048, "res", False, 1, 32),
                  (8, 48, 96, "f32", True, 0, 32), (8, 40, 320, "bf16", True, 0, 64), (5, 40, 2048, "res", True, 1, 256), (8, 48, 3328, "f32", True, 0, 160),
                  (8, 48, 512, "f32", True, 3, 32), (8, 40, 1024, "bf16", True, 3, 64), (5, 40, 2048, "res", True, 3, 256),
                  (12, 48, 2048, "res", True, 3, 160), (16, 48, 4096, "f32", True, 3, 256), (24, 48, 2048, "bf16", True, 3, 64),
                  (32, 48, 512, "res", True, 3, 32), (8, 48, 96, "f32", True, 3, 32),
                  # K = 96, the shortest sum of the module: a worst-case bound in K is loosest at large K, the twin's ratio largest here
                  (8, 40, 96, "bf16", True, 0, 32), (5, 40, 96, "res", True, 0, 64), (8, 48, 96, "bf16", True, 3, 32), (5, 48, 96, "res", True, 3, 64)]]


@pytest.mark.parametrize("c", RAND_CASES, ids=lambda c: f"{c.M}x{c.N}x{c.K}-{c.epi}-n{int(c.norm)}-p{c.packed}")
def test_random_rowwise(backend, c):
    ratios = {}
    _run(backend, c, ratios, {})
    _assert_ratios(f"rand-{c.M}x{c.N}x{c.K}-{c.epi}-n{int(c.norm)}-p{c.packed}", ratios, backend)


# ----------------------------------------------------------------------------- 4: the statistics probe
PROBE_M = (5, 8, 12, 16, 17, 24, 32)
PROBE_NSS = (32, 64, 160, 256)


def _probe_stats(M, nss, K):
    """a different positive number in every column and another set per row; rows >= M poisoned"""
    i, j = torch.arange(M, dtype=F64)[:, None], torch.arange(nss, dtype=F64)[None, :]
    ss = torch.full((_stat_rows(M), nss), POISON, dtype=F32)
    ss[:M] = ((1.0 + j * 0.37 + ((j * 7) % 11) * 1.3) * (1.0 + 0.61 * i) * K / nss / 8).to(F32)
    assert all(torch.unique(ss[r]).numel() == nss for r in range(M))
    rstd = torch.rsqrt(ss[:M].to(F64).sum(1) / K + float(torch.tensor(EPS, dtype=F32)))
    assert torch.unique(rstd.to(F32)).numel() == M
    return ss, rstd


@pytest.mark.parametrize("nss", PROBE_NSS)
@pytest.mark.parametrize("M", PROBE_M)
def test_statistics_fold_probe(backend, M, nss):
    """NORM 2 (every row class, packed = 3, fp32 output; <= 8 rows in both tile modes' fold: the diagonal mode through bf16 + power-of-two
    checks is left to the forms): out[m, n] = rstd_m W'[n, k_m] with rstd_m = rsqrt(sum of all nss columns of row m / K + eps)"""
    K, N = 512, 48
    ss, rstd = _probe_stats(M, nss, K)
    g = torch.Generator().manual_seed(M + nss)
    km = torch.randperm(K, generator=g)[:M]
    x = torch.zeros(M, K, dtype=F64)
    x[torch.arange(M), km] = 1.0
    W = _pow2(g, (N, K), -3, 3)
    nw = torch.ones(K, dtype=BF)
    dev = backend
    Wk = ops.dec_pack_weights(W.to(BF).to(dev), out_f32=True, norm_w=nw.to(dev), rows=8 if M <= 8 else 16)
    win = _Window(M, N, F32, dev)
    xd = x.to(BF).to(dev)
    rc = _lib.get_lib().call_rc("bra_dec_gemm2_packed", xd, K, ss.to(dev), nss, nw.to(dev), EPS, Wk, K, None, 0, win.win, win.win.stride(0), None, 0,
                                M, N, K, 0, 1, 3, _lib.current_stream(xd))
    assert rc == 0
    got = win.result(f"probe-{M}-{nss}").to(F64)
    r = got / W[:, km].T
    err = (r - rstd[:, None]).abs() / rstd[:, None]
    assert (err <= _tau_rstd(nss) * U32).all(), (M, nss, "rows", sorted(set(torch.nonzero(err > _tau_rstd(nss) * U32)[:, 0].tolist())), err.max().item() / U32)
    if M > 8:
        return
    # the diagonal mode's fold (rs_lds[fr & 7]): bf16 output, N = 40, K = 1024 — rstd_m W' rounded once: bf16(rstd_m) W'
    K, N = 1024, 40
    assert _mirror(M, N, K, "bf16", True, 3)["form"][:5] == (8, 1, 4, 4, "fast")
    ss, rstd = _probe_stats(M, nss, K)
    km = torch.randperm(K, generator=g)[:M]
    x = torch.zeros(M, K, dtype=F64)
    x[torch.arange(M), km] = 1.0
    W = _pow2(g, (N, K), -3, 3)
    nw = torch.ones(K, dtype=BF)
    Wk = ops.dec_pack_weights(W.to(BF).to(dev), norm_w=nw.to(dev), rows=8)
    win = _Window(M, N, BF, dev)
    xd = x.to(BF).to(dev)
    rc = _lib.get_lib().call_rc("bra_dec_gemm2_packed", xd, K, ss.to(dev), nss, nw.to(dev), EPS, Wk, K, None, 0, win.win, win.win.stride(0), None, 0,
                                M, N, K, 0, 0, 3, _lib.current_stream(xd))
    assert rc == 0
    got = win.result(f"probe-diag-{M}-{nss}").to(F64)
    tau = _tau_rstd(nss) * U32
    lo, hi = _bf(rstd * (1 - tau))[:, None] * W[:, km].T, _bf(rstd * (1 + tau))[:, None] * W[:, km].T
    assert ((got == lo) | (got == hi)).all(), (M, nss, torch.nonzero((got != lo) & (got != hi))[:6].tolist())


@pytest.mark.parametrize("nss", PROBE_NSS)
@pytest.mark.parametrize("M", (5, 8))
@pytest.mark.parametrize("K,N", [(96, 48), (320, 40)])
def test_statistics_fold_probe_in_register_norm(backend, M, nss, K, N):
    """NORM 1 (<= 8 rows, both tile modes) through a one-hot W: out[m, n] = bf16(w_k bf16(x_mk rstd_m)) = w_k x_mk bf16(rstd_m) for powers of two"""
    ss, rstd = _probe_stats(M, nss, K)
    tau = _tau_rstd(nss) * U32
    g = torch.Generator().manual_seed(M + nss + K)
    x, nw = _pow2(g, (M, K), -2, 2), _pow2(g, (K,), -1, 1).abs()
    kn = torch.randperm(K, generator=g)[:N]
    W = torch.zeros(N, K, dtype=F64)
    W[torch.arange(N), kn] = 1.0
    dev = backend
    xd, Wd, nwd = x.to(BF).to(dev), W.to(BF).to(dev), nw.to(BF).to(dev)
    for f32 in (1, 0):
        win = _Window(M, N, F32 if f32 else BF, dev)
        rc = _lib.get_lib().call_rc("bra_dec_gemm2", xd, K, ss.to(dev), nss, nwd, EPS, Wd, K, None, 0, win.win, win.win.stride(0), None, 0,
                                    M, N, K, 0, f32, _lib.current_stream(xd))
        assert rc == 0
        assert _mirror(M, N, K, "f32" if f32 else "bf16", True, 0)["form"].mode == (0 if f32 else int(K % 64 == 0))
        got = win.result(f"probe1-{M}-{nss}-{K}").to(F64)
        scale = (nw[None, :] * x)[:, kn]
        lo, hi = _bf(rstd * (1 - tau))[:, None] * scale, _bf(rstd * (1 + tau))[:, None] * scale
        ok = (got == lo) | (got == hi)
        assert ok.all(), (M, nss, K, f32, torch.nonzero(~ok)[:6].tolist())


# ----------------------------------------------------------------------------- 5: bra_row_sumsq, the packers
@pytest.mark.parametrize("K", [8, 40, 264, 2048])
@pytest.mark.parametrize("M", [1, 8, 16, 17, 32])
def test_row_sumsq(backend, M, K):
    """row_sumsq_kernel: ss[r][0] = sum of squares of row r (integers: exact), ss[r][1 .. nss) = 0 — it WRITES zeros over what was there —
    and rows >= M and columns >= nss keep the pattern"""
    g = torch.Generator().manual_seed(M + K)
    x = _randint(g, (M, K), 4).to(BF)
    nss = 32 if K < 2048 else 256
    win = _WindowAt(M, nss, F32, backend, 0, nss)                   # (rows of ss are nss apart: a dense array between two guard rows)
    xd = _wide(x, backend)
    _lib.get_lib().call("bra_row_sumsq", xd, xd.stride(0), M, K, win.win, nss, _lib.current_stream(xd))
    got = win.result(f"row_sumsq-{M}x{K}")
    want = torch.zeros(M, nss, dtype=F32)
    want[:, 0] = (x.to(F64) ** 2).sum(1).to(F32)
    _assert_bits(f"row_sumsq-{M}x{K}", got, want)


def _chunks(t):
    """the multiset of 16-byte chunks of a bf16 matrix: (sorted distinct chunks, their counts)"""
    c = t.detach().cpu().contiguous().view(torch.int16).view(-1, 8)
    return torch.unique(c, dim=0, return_counts=True)


def _same_chunks(a, b):
    (ua, ca), (ub, cb) = _chunks(a), _chunks(b)
    return ua.shape == ub.shape and torch.equal(ua, ub) and torch.equal(ca, cb)


@pytest.mark.parametrize("N,K,act,f32,rows", [(40, 1024, 0, 0, 8), (48, 96, 0, 0, 8), (48, 512, 1, 0, 8), (48, 512, 0, 1, 16), (48, 2048, 0, 0, 16), (2064, 512, 0, 0, 8)])
def test_pack_is_a_permutation_of_chunks(backend, N, K, act, f32, rows):
    """the packed image holds exactly the 16-byte chunks of W — of bf16(W * w), rounded once, with a folded norm (the ORDER is held by
    every packed case above: pack, then stream)"""
    d = _inputs(8, N, K, "rand")
    W, nw = d["W"].to(backend), d["nw"].to(backend)
    Wp = ops.dec_pack_weights(W, act=bool(act), out_f32=bool(f32), rows=rows)
    assert _same_chunks(Wp, W)
    Wf = ops.dec_pack_weights(W, act=bool(act), out_f32=bool(f32), norm_w=nw, rows=rows)
    folded = (d["W"].to(F64) * d["nw"].to(F64)[None, :]).to(BF)
    assert _same_chunks(Wf, folded) and not _same_chunks(Wf, W)


# ----------------------------------------------------------------------------- 6: fp8 weights
FP8_K0 = (512, 1024, 1536, 2048, 2560, 3072)            # 16-column tiles (SwiGLU / fp32): the six forms
FP8_K1 = (1024, 2048, 3072, 4096, 5120, 6144)           # diagonal tiles


@functools.lru_cache(maxsize=32)
def _fp8_inputs(M, N, K, vals):
    g = torch.Generator().manual_seed(977 * M + 13 * N + K + (0 if vals == "exact" else 1))
    if vals == "exact":
        x, W, res = _randint(g, (M, K), 4), _randint(g, (N, K), 7), _randint(g, (M, N), 256)
        W[torch.arange(N), torch.randint(0, K, (N,), generator=g)] = 7.0
        nw = torch.ones(K, dtype=F64)
    else:
        x, W = torch.randn(M, K, generator=g, dtype=F64) * 0.5, torch.randn(N, K, generator=g, dtype=F64) * 0.5
        res, nw = torch.randn(M, N, generator=g, dtype=F64), 1 + 0.1 * torch.randn(K, generator=g, dtype=F64)
    return {"M": M, "N": N, "K": K, "x": x.to(BF), "W": W.to(BF), "res": res.to(BF), "nw": nw.to(BF)}


def _fp8_case(dev, M, N, K, epi, folded, vals, ratios, tally):
    act, f32 = epi == "act", epi in ("f32", "f32max")
    m = _mirror(M, N, K, epi, folded, 3 if folded else 1, fp8=True)
    assert not m["refused"] and m["form"].kind == "fast"
    diag = bool(m["form"].mode)
    name = f"fp8-m{int(diag)}-{m['form'].nw}x{m['form'].nl}-{epi}-{M}x{N}x{K}-{vals}" + ("-folded" if folded else "")
    d = _fp8_inputs(M, N, K, vals)
    x, W = d["x"].to(dev), d["W"].to(dev)
    packed = ops.dec_pack_weights_fp8(W, act=act, out_f32=f32, norm_w=d["nw"].to(dev) if folded else None)
    assert packed is not None, name
    q, sc = packed
    codes = unpack_fp8_fast(q, N, K, diag).view(F8).to(F64)
    scale = sc.detach().cpu()
    if vals == "exact":
        assert (scale == 2.0 ** -6).all(), name
        assert torch.equal(codes, 64 * d["W"].to(F64)), name
    ss_in, rstd, nss = None, None, 0
    if folded:
        nss = 64
        ss_cpu, rstd = _stats({"M": M, "K": K, "x": d["x"]}, nss, 8)
        ss_in = ss_cpu.to(dev)
    win = _Window(M, N // 2 if act else N, F32 if f32 else BF, dev, "direct" if M % 2 else "lds")
    res = d["res"].to(dev) if epi == "res" else None
    ncol = 8 if diag else 16
    sw = _Window(M, m["ntiles"], F32, dev, "direct") if epi in ("res", "f32max") else None
    rc = _lib.get_lib().call_rc("bra_dec_gemm2_fp8", x, K, ss_in, nss, EPS, q, sc, res, N if res is not None else 0, win.win, win.win.stride(0),
                                sw.win if sw else None, sw.win.stride(0) if sw else 0, M, N, K, int(act), int(f32), int(folded), _lib.current_stream(x))
    assert rc == 0, (name, rc)
    got = win.result(name)
    X, R = d["x"].to(F64), d["res"].to(F64)
    Wq = codes * scale.to(F64)[:, None]
    if vals == "exact":
        acc = X @ Wq.T
        assert torch.equal(acc, X @ d["W"].to(F64).T)
        if act:
            raise AssertionError("the exact fp8 set has no SwiGLU case")
        want = acc.to(F32) if f32 else ((_bf(acc) + R).to(BF) if epi == "res" else acc.to(BF))
        if not f32:
            tally["ties"] = tally.get("ties", 0) + _ties(acc) + (_ties(_bf(acc) + R) if epi == "res" else 0)
        _assert_bits(name, got, want)
    else:
        xn = X * rstd[:, None] if folded else X
        ref, E = _bound_ref(xn, Wq, K, _what(epi), R, c_epi=3, tau=_tau_rstd(nss) if folded else 0.0)
        key = f"{'f8n2' if folded else 'f8'}_{_what(epi)}"
        ratios[key] = max(ratios.get(key, 0.0), _ratio((got.to(F64) - ref).abs(), E))
    if epi == "res":
        tally["ss_exact"] = tally.get("ss_exact", 0) + _check_ss(name, sw.result(name + " ss_out"), got, ncol, m["ntiles"])
    if epi == "f32max":
        _assert_bits(name + " tile maxima", sw.result(name + " tile maxima"), got.view(M, m["ntiles"], 16).amax(-1))


@pytest.mark.parametrize("i", range(6))
def test_fp8_rowwise(backend, i):
    """bra_dec_pack_weights_fp8 + bra_dec_gemm2_fp8 at the six (waves, chunks) forms of both tile modes: scales 2^-6 and codes 64 W asserted,
    the projection bit for bit; per-column scales that differ (random rows) under the bound against the decoded codes"""
    ratios, tally = {}, {}
    K0, K1 = FP8_K0[i], FP8_K1[i]
    M = (1, 5, 8)[i % 3]
    _fp8_case(backend, M, 48, K0, "f32max", False, "exact", ratios, tally)
    _fp8_case(backend, M, 40, K1, "res", False, "exact", ratios, tally)
    _fp8_case(backend, 8, 40, K1, "bf16", False, "exact", ratios, tally)
    _fp8_case(backend, 8, 48, K0, "f32", True, "rand", ratios, tally)
    _fp8_case(backend, 8, 48, K0, "f32", False, "rand", ratios, tally)
    _fp8_case(backend, 8, 40, K1, "res", False, "rand", ratios, tally)
    _fp8_case(backend, 8, 40, K1, "bf16", True, "rand", ratios, tally)
    assert tally["ties"] > 0 and tally["ss_exact"] > 0
    _assert_ratios(f"fp8-{K0}-{K1}", ratios, backend)


# ----------------------------------------------------------------------------- 7: the first generation (k_decfused.hip: bra_dec_gemm)
# (M, N, K): N = 40 narrow (8-column workgroups), 44 / 4107 sixteen columns with a ragged tail; M <= 8 and 9 .. 16: the two prologue heights;
# K = 96 (one batch of eight steps per wave, clamped), 1056 (33 steps: wave 0 runs a second batch), 4160 (130 steps)
V1 = [(5, 40, 96), (8, 44, 1056), (12, 40, 1056), (16, 44, 96), (1, 44, 4160), (9, 40, 4160), (8, 4107, 96)]
V1_RAND = [(5, 40, 96), (12, 44, 1056), (16, 40, 4160), (8, 44, 4160)]


def _v1_mirror(N, act):
    return (not act) and (N + 15) // 16 < 256 and N % 8 == 0


def _v1_call(dev, d, epi, norm, layout="lds", strided=False, name=""):
    M, N, K = d["M"], d["N"], d["K"]
    act, f32 = epi == "act", epi == "f32"
    x = _wide(d["x"], dev) if strided else d["x"].to(dev)
    W = _wide(d["W"], dev) if strided else d["W"].to(dev)
    win = _Window(M, N // 2 if act else N, F32 if f32 else BF, dev, layout)
    res = None
    if epi == "res":
        rw = _WindowAt(M, N, BF, dev, 4, N + 4 + (-(N + 4)) % 8 + 4)
        rw.buf[1:1 + M, 4:4 + N] = d["res"].to(dev)
        res = rw.win
    _lib.get_lib().call("bra_dec_gemm", x, x.stride(0), d["nw"].to(dev) if norm else None, EPS, W, W.stride(0), res, res.stride(0) if res is not None else 0,
                        win.win, win.win.stride(0), M, N, K, int(act), int(f32), _lib.current_stream(x))
    return win.result(name)


def _v1_tau(K):
    """a thread adds 8 ceil(K / 2048) squares in sequence, six butterfly steps, three additions across the waves"""
    return (8 * -(-K // 2048) + 9 + 5) / 2 + 2


@pytest.mark.parametrize("M,N,K", V1)
def test_first_generation_exact(backend, M, N, K):
    """bra_dec_gemm without norm: both tile widths, both prologue heights, residual / fp32 / SwiGLU epilogues, bit for bit"""
    d = _inputs(M, N, K, "exact")
    acc = d["x"].to(F64) @ d["W"].to(F64).T
    R = d["res"].to(F64)
    assert _v1_mirror(N, False) == (N == 40)
    ties = 0
    for j, (epi, want) in enumerate((("bf16", acc.to(BF)), ("res", (_bf(acc) + R).to(BF)), ("f32", acc.to(F32)))):
        name = f"v1-{M}x{N}x{K}-{epi}"
        _assert_bits(name, _v1_call(backend, d, epi, False, ("lds", "direct")[(j + M) % 2], strided=bool((j + N) % 2), name=name), want)
    ties = _ties(acc) + _ties(_bf(acc) + R)
    assert ties > 0
    da, _, _, twin = _swiglu_case(M, 48, K, 0, 0)
    _assert_swiglu(f"v1-{M}x48x{K}-act", _v1_call(backend, da, "act", False, name="v1-act"), twin)
    # the same epilogue behind the RMSNorm prologue: x = +-2^j, so its sum of squares is exact and bf16(w bf16(x rstd)) = w x bf16(rstd)
    for attempt in range(8):
        da = _inputs(M, 48, K, "act", attempt)
        rstd = torch.rsqrt((da["x"].to(F64) ** 2).mean(1) + float(torch.tensor(EPS, dtype=F32)))
        if _near(rstd, _v1_tau(K) * U32 * rstd).any():
            continue
        twin = _swiglu_twin(da, 1, rstd, _v1_tau(K))
        if (twin[1] | twin[2]).float().mean().item() <= NEAR_CAP:
            break
    else:
        raise AssertionError("no SwiGLU input set within the cap")
    _assert_swiglu(f"v1-{M}x48x{K}-act-norm", _v1_call(backend, da, "act", True, name="v1-act-norm"), twin)


@pytest.mark.parametrize("M,N,K", V1_RAND)
def test_first_generation_random(backend, M, N, K):
    """bra_dec_gemm with its RMSNorm prologue (bf16(w * bf16(x * rstd)) into LDS; rstd from its own sum of squares) and without, under the bound"""
    d = _inputs(M, N, K, "rand")
    X, W64, R = d["x"].to(F64), d["W"].to(F64), d["res"].to(F64)
    rstd = torch.rsqrt((X ** 2).mean(1) + float(torch.tensor(EPS, dtype=F32)))
    xn = X * rstd[:, None] * d["nw"].to(F64)
    ratios = {}
    for norm in (True, False):
        for epi in ("f32", "bf16", "res"):
            name = f"v1-{M}x{N}x{K}-{epi}-rand-n{int(norm)}"
            got = _v1_call(backend, d, epi, norm, name=name)
            ref, E = _bound_ref(xn, W64, K, epi, R, act_round=2, tau=_v1_tau(K)) if norm else _bound_ref(X, W64, K, epi, R)
            key = f"n{int(norm)}_{epi}"
            ratios[key] = max(ratios.get(key, 0.0), _ratio((got.to(F64) - ref).abs(), E))
    _assert_ratios(f"v1-{M}x{N}x{K}", ratios, backend)


# ----------------------------------------------------------------------------- the twin
def _twin(d, epi, norm_kind, rstd64, fp8=False):
    """float32, no project code: sequential accumulation over k, .to(bfloat16) at the documented rounding points"""
    x, W, nw = d["x"].to(F32), d["W"].to(F32), d["nw"].to(F32)
    rstd = rstd64.to(F32)[:, None] if rstd64 is not None else None
    scale = None
    if norm_kind == 2 or (fp8 and norm_kind):
        W = (W * nw[None, :]).to(BF).to(F32) if not fp8 else W * nw[None, :]
    if fp8:
        amax = W.abs().amax(1)
        scale = amax * torch.tensor(1.0 / 448.0, dtype=F32)
        W = (W * (1.0 / scale)[:, None]).to(F8).to(F32)
    if norm_kind == 1:
        x = (nw[None, :] * (x * rstd).to(BF).to(F32)).to(BF).to(F32)
    v = _seq_matmul32(x, W)
    if norm_kind == 2 or (fp8 and norm_kind):
        v = v * rstd
    if fp8:
        v = v * scale[None, :]
    if epi == "f32":
        return v, (W.to(F64) * scale.to(F64)[:, None] if fp8 else None)
    v = v.to(BF)
    if epi == "res":
        v = (v.to(F32) + d["res"].to(F32)).to(BF)
    return v, (W.to(F64) * scale.to(F64)[:, None] if fp8 else None)


FP8_RAND = [(M, N, K, epi, folded) for i in range(6) for (M, N, K, epi, folded) in [
    (8, 48, FP8_K0[i], "f32", True), (8, 48, FP8_K0[i], "f32", False), (8, 40, FP8_K1[i], "res", False), (8, 40, FP8_K1[i], "bf16", True)]]


def _twin_worst():
    worst, where = dict.fromkeys(TWIN_WORST, 0.0), {}

    def note(key, name, got, ref, E):
        w = _ratio((got.to(F64) - ref).abs(), E)
        if w > worst[key]:
            worst[key], where[key] = w, name

    for c in RAND_CASES:
        d = _inputs(c.M, c.N, c.K, "rand")
        X, W64, R = d["x"].to(F64), d["W"].to(F64), d["res"].to(F64)
        n = 0 if not c.norm else (2 if c.packed & 2 else 1)
        rstd = _stats(d, c.nss, _stat_rows(c.M))[1] if n else None
        what = _what(c.epi)
        if n:
            ref, E = _bound_ref(X * rstd[:, None] * d["nw"].to(F64), W64, c.K, what, R, act_round=2 if n == 1 else 1, tau=_tau_rstd(c.nss))
        else:
            ref, E = _bound_ref(X, W64, c.K, what, R)
        note(f"n{n}_{what}", f"{c.M}x{c.N}x{c.K}", _twin(d, what, n, rstd)[0], ref, E)
    for (M, N, K) in V1_RAND:
        d = _inputs(M, N, K, "rand")
        X, W64, R = d["x"].to(F64), d["W"].to(F64), d["res"].to(F64)
        rstd = torch.rsqrt((X ** 2).mean(1) + float(torch.tensor(EPS, dtype=F32)))
        for epi in ("f32", "bf16", "res"):
            ref, E = _bound_ref(X * rstd[:, None] * d["nw"].to(F64), W64, K, epi, R, act_round=2, tau=_v1_tau(K))
            note(f"n1_{epi}", f"v1-{M}x{N}x{K}", _twin(d, epi, 1, rstd)[0], ref, E)
            ref, E = _bound_ref(X, W64, K, epi, R)
            note(f"n0_{epi}", f"v1-{M}x{N}x{K}", _twin(d, epi, 0, None)[0], ref, E)
    for (M, N, K, epi, folded) in FP8_RAND:
        d = _fp8_inputs(M, N, K, "rand")
        X, R = d["x"].to(F64), d["res"].to(F64)
        rstd = _stats({"M": M, "K": K, "x": d["x"]}, 64, 8)[1] if folded else None
        got, Wq = _twin(d, epi, 2 if folded else 0, rstd, fp8=True)
        ref, E = _bound_ref(X * rstd[:, None] if folded else X, Wq, K, epi, R, c_epi=3, tau=_tau_rstd(64) if folded else 0.0)
        note(f"{'f8n2' if folded else 'f8'}_{epi}", f"fp8-{M}x{N}x{K}", got, ref, E)
    return worst, where


def test_twin_ratio_is_the_recorded_one():
    """MARGIN's origin, reproducible without a GPU and without project code"""
    worst, where = _twin_worst()
    print(f"\n[dec-proj] twin worst ratios { {k_: float(f'{v_:.4g}') for k_, v_ in worst.items()} } at {where}")
    for k_ in TWIN_WORST:
        assert math.isfinite(worst[k_]) and abs(worst[k_] - TWIN_WORST[k_]) <= 0.01 * TWIN_WORST[k_] + 5e-5, (k_, worst[k_], where.get(k_))
        assert MARGIN[k_] == 2 * TWIN_WORST[k_]
