"""Decode attention, row by row against float64: bra_dec_attn_one (k_decattn.hip / bra_decattn.h), the first-generation path
bra_dec_attn_both / bra_dec_attn_shared / bra_dec_attn_partial + bra_attn_decode_merge (k_decfused.hip, k_attn.hip), ops.attn_decode, and the merge kernel
alone on synthetic partials.  tests/test_kernels.py holds these kernels by one Frobenius ratio over all B * Hq rows: one wrong
(sequence, head) row, a dropped chunk of small softmax weight, a wrong weight register in the merge's tail loop pass there.

Reference (_norm_rope64, _row_ref; no project kernel is called): per row (b, hq) the key list = prompt keys of its prompt, its cached
completion keys, the new key; p = softmax(scale K q), ref = p V, A_d = sum_j p_j |v_jd| — all float64.  q and the new k are the
normalised, rotated projections rounded to bf16 where the kernels round them: after x * rstd, after * w, after the rotation.

Bound, every element of every row:      |got - ref| <= (T_path + 2 Delta_row + c) A_d        U = 2^-9

  path                                    rounding points                                            T_path   Delta_row over
  bra_dec_attn_one                        q scale log2e -> bf16 for the MFMA (one_item), p -> bf16     3 U      prompt + completion keys
    (one_item / one_newkey / merge_one)   for the PV MFMA (U), bf16 output (2 U); the new key's score           (the new key's score uses
                                          and the merge are fp32                                                 the unrounded fp32 q)
  bra_dec_attn_both + merge               prompt keys: dec_attn_shared_body, as one_item; completion   3 U      prompt keys
                                          and new key: dec_attn_partial_body, fp32 q and p; bf16 out
  bra_dec_attn_partial + merge            dec_attn_partial_body only: fp32 q and p; bf16 output        2 U      -
  ops.attn_decode                         attn_decode_partial_kernel: fp32 q scale and p; bf16 output  2 U      -
  bra_attn_decode_merge alone             fp32 weights and sums; bf16 output                           2 U      -   (A_d = sum_c w_c |O_cd| / l)

  The bf16 OUTPUT counts 2 U = 2^-8, not U.  bfloat16 keeps 8 significand bits: the spacing in [1, 2) is 2^-7, a correctly rounded
  value just above a power of two is off by up to 2^-8 of itself (U is the figure at the top of a binade).  The first derivation
  counted U; the merge of a single chunk (A_d = |ref| exactly, the only rounding the output's) then exceeded it by 0.97 U with
  correctly rounded results — e.g. ref 1.019591 -> 1.0234375 — and c would have had to be 4 x that, above U: the missing piece of the
  derivation was this factor, from the number format, not a tolerance for the kernel.  The p -> bf16 term stays U: the largest
  probability of a chunk is exactly 1, the others' rounding errors do not align.
  Delta_row = U scale max_j sum_i |q_i k_ji| over the valid keys j that go through an MFMA: each element of q scale log2e moves by a
  relative U, a score by at most Delta_row, a normalised probability by at most a factor exp(2 Delta_row).
  c covers fp32 accumulation and exp2.  Measured: the worst excess  max(|got - ref| / A_d - T_path - 2 Delta_row)  of the unmodified
  kernels over every case of this module, per family; c = 4 x the largest of the two backends' excess (the device's v_exp_f32 and
  MFMA summation order are not the emulator's libm and loop order) and of the floor 2^-14, which is what fp32 alone explains: 513
  accumulated slots (or 64 keys + 256 slots) at 2^-24 each and an exp2 argument of magnitude <= 64 known to 2^-24 of itself.

      path (family)                                  emulator       MI355X
      bra_dec_attn_one (attn)                        -2.170e-02     -2.170e-02
      bra_dec_attn_both + merge (attn)               -2.782e-02     -2.782e-02
      shared + partial + merge (attn)                -2.782e-02     -2.782e-02
      bra_dec_attn_partial + merge (attn)            -5.260e-04     -5.260e-04
      ops.attn_decode (attn)                         -1.280e-03     -1.280e-03
      bra_attn_decode_merge alone (merge)            -4.966e-05     -4.966e-05
      c = 4 x max(2^-14, worst) = 2^-12 = 2.44e-04 for both families

  A negative excess: the derived terms alone cover the kernel at its worst element (with 2 Delta_row near 0.03 for unit-normal
  rows of the MFMA paths they are far from tight there; the adversarial rows and the merge-alone cases are where a fault shows).
  c < U is asserted: a larger c would mean a rounding point is missing from the derivation.

Side effects, exactly: the appended K row equals the reference's rounded new k bit for bit — except where the reference itself marks
the element boundary-near (its float64 value before one of the roundings lies within the fp32 error of that product of a bf16 rounding
boundary; tests/test_layer_glue_rowwise.py's criterion for the same norm + rotation): one bf16 ulp there, and at most NEAR_CAP of the
elements may carry the mark.  The appended V is a copy: bit for bit.  Every other cache element, the pad columns of o and the partial
slots behind the last one the merge reads keep their bits (NaN pre-fill for the partials, so a finite result also shows that no
unwritten slot was read).  Buffers a clamped or off-by-one index could reach are allocated and poisoned: NaN where nothing may be
read (K rows past the last key, columns past the pitch), finite sentinels where a zero-weight operand is read (V^T columns
between the last key and the end of its 64-key chunk; row t of the first-generation caches before the append, where clamped indices land).

Values: `rand` = unit normals; the adversarial kinds of ADV (one key of the last prompt chunk ~30 above the rest, the new key dominant,
equal scores from identical keys, a chunk that underflows against the global maximum, |v| from 2^-6 to 2^6 across keys, q-norm
weights x 6); test_adv_reference_is_finite checks on the CPU that the float64 reference is finite with A_d > 0 for each.
"""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bioreason_amd import ops, _lib                                                      # noqa: E402
from bioreason_amd._lib import current_stream                                             # noqa: E402
from test_layer_glue_rowwise import _near, _ord, _tau_rstd, NEAR_CAP                       # noqa: E402

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0 ** -9
U32 = 2.0 ** -24
EPS = 1e-6
NEG = -1.0e30

# worst excess over the derived terms: path -> (family, emulator, MI355X); unmodified kernels, every case of this module (the docstring's table)
EXCESS = {
    "one": ("attn", -2.170e-02, -2.170e-02),
    "both": ("attn", -2.782e-02, -2.782e-02),
    "three": ("attn", -2.782e-02, -2.782e-02),
    "partial": ("attn", -5.260e-04, -5.260e-04),
    "attn_decode": ("attn", -1.280e-03, -1.280e-03),
    "merge": ("merge", -4.966e-05, -4.966e-05),
}
C_FLOOR = 2.0 ** -14
C_ = {fam: 4.0 * max([C_FLOOR] + [max(e, h) for f, e, h in EXCESS.values() if f == fam]) for fam in ("attn", "merge")}
ADV = ["dom_prompt", "dom_new", "equal", "underflow", "mixed_v", "qw6"]


def test_c_is_below_the_smallest_derived_term():
    for fam, c in C_.items():
        assert 0.0 <= c < U, (fam, c)


# ----------------------------------------------------------------------------- reference
def _f32(v):
    return float(torch.tensor(v, dtype=F32))


def _bf(x):
    return x.to(F32).to(BF).to(F64)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def _norm_rope64(x, w, cos, sin):
    """per-head RMSNorm (weight w) + rotate-half RoPE of x [..., hd] (float64 of bf16) with cos / sin [..., hd/2]: float64, bf16
    roundings after x * rstd, after * w and (the caller's) after the rotation -> (value before the last rounding, boundary-near mark)"""
    hd = x.shape[-1]
    half = hd // 2
    r = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + _f32(EPS))
    inner = x * r
    near = _near(inner, U32 * (_tau_rstd(8, int(math.log2(hd))) + 1) * inner.abs())
    y = _bf(w * _bf(inner))                                 # a product of two bf16 numbers is exact in fp32: no mark
    x1, x2 = y[..., :half], y[..., half:]
    o1, o2 = x1 * cos - x2 * sin, x2 * cos + x1 * sin
    nin = near[..., :half] | near[..., half:]
    n1 = _near(o1, U32 * ((x1 * cos).abs() + (x2 * sin).abs() + o1.abs())) | nin
    n2 = _near(o2, U32 * ((x2 * cos).abs() + (x1 * sin).abs() + o2.abs())) | nin
    return torch.cat([o1, o2], -1), torch.cat([n1, n2], -1)


def _row_ref(q, K, V, valid, mfma, scale):
    """one row in float64: -> (ref [hd], A [hd], Delta).  K, V [n, hd]; valid, mfma [n] bool"""
    assert bool(valid.any()), "a row without a valid key"
    s = scale * (K @ q)
    s = torch.where(valid, s, torch.full_like(s, -math.inf))
    p = torch.softmax(s, 0)
    sel = valid & mfma
    delta = U * scale * float((K[sel].abs() @ q.abs()).max()) if bool(sel.any()) else 0.0
    return p @ V, p @ V.abs(), delta


WORST = {}                 # family -> worst excess seen in this process (printed per case: `pytest -s`)


def _check_rows(name, fam, backend, got, rows, T):
    """got [n, hd] float64; rows: n tuples (label, ref, A, Delta).  Every element of every row."""
    worst, where = -math.inf, None
    bad = []
    for i, (label, ref, A, delta) in enumerate(rows):
        assert bool(torch.isfinite(ref).all()) and bool((A > 0).all()), (name, label, "reference")
        g = got[i]
        assert bool(torch.isfinite(g).all()), (name, label, "non-finite output")
        ratio = (g - ref).abs() / A
        ex = float(ratio.max()) - T - 2 * delta
        if ex > worst:
            worst, where = ex, label
        lim = (T + 2 * delta + C_[fam]) * A
        if bool(((g - ref).abs() > lim).any()):
            d = int(((g - ref).abs() / lim).argmax())
            bad.append((label, d, float(g[d]), float(ref[d]), float(ratio[d]), T + 2 * delta + C_[fam]))
    key = (fam, "hip" if backend.type == "cuda" else "emu")
    WORST[key] = max(WORST.get(key, -math.inf), worst)
    print(f"\n[dec-attn-rowwise] {name}: rows {len(rows)} excess {worst:+.3e} at {where} (family worst {WORST[key]:+.3e})")
    assert not bad, (name, "row, dim, got, ref, |err|/A, bound", bad[:6])


def _assert_appended_k(name, got_bf, pre, near):
    got = got_bf.detach().cpu()
    want = pre.to(F32).to(BF)
    d = (_ord(got) - _ord(want)).abs()
    assert int(near.sum()) <= max(2, NEAR_CAP * near.numel()), (name, int(near.sum()), near.numel())
    ok = (d == 0) | ((d == 1) & near)
    assert bool(ok.all()), (name, "appended K", torch.nonzero(~ok)[:6].tolist())


# ----------------------------------------------------------------------------- inputs of one shared-prefix step
class _Step:
    pass


def _rope_tables(hd, npos):
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=F64) / hd))
    ang = torch.arange(npos, dtype=F64)[:, None] * inv[None]
    return ang.cos().to(F32), ang.sin().to(F32)


def _make(hd, Hq, Hkv, R, copies, P, C, t, values="rand", pad=(), seed=0):
    """CPU tensors (bf16 values) of one decode step of B = R * copies sequences + its float64 q / new k"""
    s = _Step()
    s.hd, s.Hq, s.Hkv, s.R, s.copies, s.P, s.C, s.t, s.values = hd, Hq, Hkv, R, copies, P, C, t, values
    s.B, s.G, s.scale = R * copies, Hq // Hkv, hd ** -0.5
    B = s.B
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * P + 131 * t + 17 * hd + Hq + 3 * copies)
    rn = lambda *sh: torch.randn(*sh, generator=g, dtype=F32)
    adv = values != "rand"
    q = rn(B, Hq, hd)
    if adv:                                    # one direction for every row (a key can then dominate every row at once)
        q = rn(1, 1, hd) + 0.15 * q
    k, v = rn(B, Hkv, hd), rn(B, Hkv, hd)
    qw, kw = 1.0 + 0.1 * rn(hd), 1.0 + 0.1 * rn(hd)
    if values == "qw6":
        qw = 6.0 * qw
    if values == "dom_new":                    # raw k = raw q of the group's first head, k-norm weight 3 x the q-norm weight
        k = q.expand(B, Hq, hd)[:, ::s.G].clone()
        kw = 3.0 * qw
    kp, vp = rn(R, Hkv, P, hd), rn(R, Hkv, P, hd)
    kold, vold = rn(B, Hkv, t, hd), rn(B, Hkv, t, hd)
    s.cos, s.sin = _rope_tables(hd, P + C + 8)
    s.pos = (torch.full((B,), P + t) if adv else torch.arange(B) % 5 + P + t - 2).clamp_min(0).to(torch.int32)
    s.qw, s.kw = qw.to(BF), kw.to(BF)
    s.qkv = torch.cat([q.expand(B, Hq, hd).reshape(B, -1), k.reshape(B, -1), v.reshape(B, -1)], 1).to(BF).contiguous()
    s.pmask = torch.ones(R, P, dtype=torch.uint8)
    for r, n in enumerate(pad):
        assert n < P
        s.pmask[r, :n] = 0
    # ---- float64 q / new k / new v
    x = s.qkv.to(F64).view(B, Hq + 2 * Hkv, hd)
    c_, s_ = s.cos[s.pos.long()].to(F64)[:, None], s.sin[s.pos.long()].to(F64)[:, None]
    q_pre, _ = _norm_rope64(x[:, :Hq], s.qw.to(F64), c_, s_)
    s.k_pre, s.k_near = _norm_rope64(x[:, Hq:Hq + Hkv], s.kw.to(F64), c_, s_)
    s.qn, s.kn, s.vn = _bf(q_pre), _bf(s.k_pre), s.qkv.view(B, Hq + 2 * Hkv, hd)[:, Hq + Hkv:]
    # ---- adversarial keys / values
    if adv:
        qbar = s.qn.mean((0, 1))
        u = (qbar / (s.scale * qbar.pow(2).sum())).to(F32)           # scale q . u ~ 1 for every row
        npc = (P + 63) // 64
        if values == "underflow":
            if npc >= 2:
                kp[:, :, :64] = -150.0 * u
            elif t >= 1:
                kold[:, :, :min(t, 64)] = -150.0 * u
        if values in ("dom_prompt", "underflow"):
            kp[:, :, max(P - 4, 0)] = 30.0 * u                        # in the last prompt chunk, never padded
        if values == "equal":
            kvec = rn(hd)
            kp[:], kold[:] = kvec, kvec
        if values == "mixed_v":
            vp *= (2.0 ** ((torch.arange(P) % 13) - 6.0))[:, None]
            vold *= (2.0 ** ((torch.arange(t) * 5 % 13) - 6.0))[:, None]
    s.kp, s.vp, s.kold, s.vold = kp.to(BF), vp.to(BF), kold.to(BF), vold.to(BF)
    return s


def _step_rows(s, mfma_completion):
    """the float64 rows of a step: (label, ref, A, Delta) per (b, hq)"""
    rows = []
    for b in range(s.B):
        r = b // s.copies
        for hq in range(s.Hq):
            h = hq // s.G
            K = torch.cat([s.kp[r, h].to(F64), s.kold[b, h].to(F64), s.kn[b, h][None]], 0)
            V = torch.cat([s.vp[r, h].to(F64), s.vold[b, h].to(F64), s.vn[b, h].to(F64)[None]], 0)
            valid = torch.cat([s.pmask[r].bool(), torch.ones(s.t + 1, dtype=torch.bool)])
            assert bool(valid[-1]), "the new key is always valid"
            mfma = torch.cat([torch.ones(s.P, dtype=torch.bool), torch.full((s.t,), bool(mfma_completion)), torch.zeros(1, dtype=torch.bool)])
            rows.append(((b, hq),) + _row_ref(s.qn[b, hq], K, V, valid, mfma, s.scale))
    return rows


def _prompt_buffers(s, dev, strided=False, vt_extra=0):
    """-> (kp view args, vtp args): K rows past P and V^T columns past the pitch NaN, V^T columns P .. pitch a finite sentinel"""
    R, Hkv, P, hd = s.R, s.Hkv, s.P, s.hd
    if strided:
        ss, sh = 2 * hd, (P + 1) * 2 * hd + 8
        sr = Hkv * sh + 16
        buf = torch.full((R * sr + 8,), float("nan"), dtype=BF)
        kv = buf.as_strided((R, Hkv, P, hd), (sr, sh, ss, 1))
        kv.copy_(s.kp)
    else:
        ss, sh, sr = hd, P * hd, Hkv * P * hd
        buf = torch.full((R * sr + 8 * hd,), float("nan"), dtype=BF)
        buf[:R * sr] = s.kp.reshape(-1)
    pitch = (P + 63) // 64 * 64
    vsd = pitch + vt_extra
    vtp = torch.full((R, Hkv, hd, vsd), float("nan"), dtype=BF)
    vtp[..., :pitch] = 64.0
    vtp[..., :P] = s.vp.transpose(2, 3)
    return (buf.to(dev), sr, sh, ss), (vtp.to(dev), Hkv * hd * vsd, hd * vsd, vsd)


# ----------------------------------------------------------------------------- bra_dec_attn_one
def _run_one(s, dev, use_mask=True, use_rows=True, via_dev=False, strided=False, vt_extra=0, ldo_extra=0, cp_extra=0, nslot=None, host_t=None,
             nslot_arg=None, out=None):
    """one call of bra_dec_attn_one on a step; -> namespace of the buffers after the call"""
    B, Hq, Hkv, hd, P, C, t = s.B, s.Hq, s.Hkv, s.hd, s.P, s.C, s.t
    Nq, Nkv = Hq * hd, Hkv * hd
    o_ = out if out is not None else _Step()
    (kp, sr, sh, ss), (vtp, vsr, vsh, vsd) = _prompt_buffers(s, dev, strided, vt_extra)
    cp = (C + 63) // 64 * 64 + cp_extra
    kc = torch.full((B, Hkv, C, hd), float("nan"), dtype=BF)           # rows >= t are never read (clamped to t - 1)
    vct = torch.full((B, Hkv, hd, cp), 5.5, dtype=BF)                  # columns t .. end of the chunk are zero-weight MFMA operands
    kc[:, :, :t] = s.kold
    vct[:, :, :, :t] = s.vold.transpose(2, 3)
    o_.kc0, o_.vct0 = kc.clone(), vct.clone()
    npc = (P + 63) // 64
    o_.nslot = nslot if nslot is not None else npc + (C + 63) // 64 + 1
    o_.part_o = torch.full((B * Hq, o_.nslot, hd), float("nan"), dtype=F32, device=dev)
    o_.part_ml = torch.full((B * Hq, o_.nslot, 2), float("nan"), dtype=F32, device=dev)
    ldo = Nq + ldo_extra
    o_.o = torch.full((B, ldo), 3.0, dtype=BF, device=dev)
    rope_rows = torch.cat([s.cos[s.pos.long()], s.sin[s.pos.long()]], -1).contiguous().to(dev) if use_rows else None
    t_dev = torch.tensor([t], dtype=torch.int32, device=dev) if via_dev else None
    o_.kc, o_.vct = kc.to(dev), vct.to(dev)
    keep = (s.qkv.to(dev), s.qw.to(dev), s.kw.to(dev), s.cos.to(dev), s.sin.to(dev), s.pos.to(dev), s.pmask.to(dev))
    th = host_t if host_t is not None else (C - 1 if via_dev else t)
    _lib.get_lib().call("bra_dec_attn_one", keep[0], Nq + 2 * Nkv, keep[1], keep[2], keep[3], keep[4], keep[5], rope_rows, kp, sr, sh, ss,
                        vtp, vsr, vsh, vsd, keep[6] if use_mask else None, o_.kc, o_.vct, cp, o_.part_o, o_.part_ml, nslot_arg if nslot_arg is not None else o_.nslot, o_.o, ldo,
                        s.R, s.copies, Hq, Hkv, hd, P, C, th, EPS, s.scale, t_dev, current_stream(keep[0]))
    if dev.type == "cuda":
        torch.cuda.synchronize()
    return o_


def _check_one(name, s, o_, backend):
    B, Hq, Hkv, hd, P, C, t = s.B, s.Hq, s.Hkv, s.hd, s.P, s.C, s.t
    Nq = Hq * hd
    o = o_.o.cpu()
    assert bool((o[:, Nq:].float() == 3.0).all()), (name, "pad columns of o written")
    _check_rows(name, "attn", backend, o[:, :Nq].to(F64).reshape(B * Hq, hd), _step_rows(s, True), 3 * U)
    # ---- caches: the appended row / column, everything else unchanged
    kc, vct = o_.kc.cpu(), o_.vct.cpu()
    _assert_appended_k(name, kc[:, :, t], s.k_pre, s.k_near)
    assert torch.equal(_bits(vct[:, :, :, t]), _bits(s.vn)), (name, "appended V^T column")
    kc0, vct0 = o_.kc0.clone(), o_.vct0.clone()
    kc0[:, :, t], vct0[:, :, :, t] = kc[:, :, t], vct[:, :, :, t]
    assert torch.equal(_bits(kc), _bits(kc0)) and torch.equal(_bits(vct), _bits(vct0)), (name, "cache elements besides the append changed")
    # ---- partial slots: [0, npc + ceil(t / 64)] written and finite, the rest still NaN
    nsl = (P + 63) // 64 + (t + 63) // 64 + 1
    po, pml = o_.part_o.cpu(), o_.part_ml.cpu()
    assert bool(torch.isfinite(po[:, :nsl]).all()) and bool(torch.isfinite(pml[:, :nsl]).all()), (name, "a slot the merge reads is not finite")
    assert bool(torch.isnan(po[:, nsl:]).all()) and bool(torch.isnan(pml[:, nsl:]).all()), (name, "a slot past the new key's was written")


def _with_adv(geoms, always=()):
    """every geometry with rand; the adversarial kinds cycled over the geometries (each kind at least once), `always` kinds at every one"""
    out = [g + ("rand",) for g in geoms]
    for i in range(max(len(geoms), len(ADV))):
        out.append(geoms[i % len(geoms)] + (ADV[i % len(ADV)],))
    for g in geoms:
        out += [g + (kind,) for kind in always if g + (kind,) not in out]
    return out


def _one(backend, name, hd, Hq, Hkv, R, copies, P, C, t, values, pad=(), **kw):
    s = _make(hd, Hq, Hkv, R, copies, P, C, t, values, pad)
    o_ = _run_one(s, backend, **kw)
    _check_one(f"one-{name}-{values}", s, o_, backend)
    return s, o_


# merge thresholds: nsl = npc + ceil(t / 64) + 1 around PRE * PR (48 at head dim 128, 96 at 64), the tail loop's passes (16 / 32 slots)
# and the weight registers' 64-slot ranges.  Hq = Hkv = R = copies = 1, C = 64, t = 1: npc = nsl - 2; a ragged last prompt chunk.
# dom_new puts the weight on the LAST slot, dom_prompt on slot npc - 1: both at every threshold.
MERGE_GEOMS = [(128, n) for n in (47, 48, 49, 64, 65, 128, 129, 192, 256)] + [(64, n) for n in (95, 96, 97, 128, 129)]


@pytest.mark.parametrize("hd,nsl,values", _with_adv(MERGE_GEOMS, always=("dom_new", "dom_prompt")))
def test_one_merge_thresholds(backend, hd, nsl, values):
    P = 64 * (nsl - 2) - 5
    s, o_ = _one(backend, f"merge-hd{hd}-nsl{nsl}", hd, 1, 1, 1, 1, P, 64, 1, values)
    assert o_.nslot == nsl


CHUNK_GEOMS = [(P, t) for P in (1, 63, 64, 65) for t in (0, 1, 63, 64, 65, 127, 128)] + [(65, 191)]


@pytest.mark.parametrize("P,t,values", _with_adv(CHUNK_GEOMS))
def test_one_chunk_edges(backend, P, t, values):
    hd, Hq = (128, 4) if (P + t) % 2 else (64, 2)
    _one(backend, f"edge-P{P}-t{t}", hd, Hq, 2, 2, 2, P, 192, t, values, pad=(min(3, P - 1),))


VIRT_GEOMS = [(c_, G, R) for (c_, G) in ((8, 4), (6, 4), (5, 4), (16, 2), (32, 1)) for R in (1, 2)]


@pytest.mark.parametrize("copies,G,R,values", _with_adv(VIRT_GEOMS))
def test_one_virtual_prompts(backend, copies, G, R, values):
    """more than 16 query rows per kv-head: virtual prompt r reads the K / V^T / mask of prompt r / rsplit (the prompts differ)"""
    hd = 128 if G == 4 else 64
    _one(backend, f"virt-c{copies}-G{G}-R{R}", hd, 2 * G, 2, R, copies, 70, 128, 66, values, pad=(5, 0)[:R])


def test_one_refuses_32_heads_per_group(backend):
    s = _make(64, 32, 1, 1, 1, 70, 64, 1)
    with pytest.raises(_lib.KernelError) as e:
        _run_one(s, backend)
    assert e.value.status == _lib.BRA_ERR_UNSUPPORTED


PAD_GEOMS = [(pad,) for pad in (0, 13, 64, 70, 128, None)]


@pytest.mark.parametrize("pad,values", _with_adv(PAD_GEOMS))
def test_one_left_padding(backend, pad, values):
    """prompt 0 padded (whole chunks at 64, 70, 128: m = -1e30, l = 0 for them), prompt 1 not; None: no mask passed"""
    _one(backend, f"pad{pad}", 128, 4, 2, 2, 2, 200, 128, 70, values, pad=(pad or 0, 0), use_mask=pad is not None)


TDEV_GEOMS = [(td,) for td in (0, 1, 64, 70)]


@pytest.mark.parametrize("td,values", _with_adv(TDEV_GEOMS))
def test_one_device_side_t(backend, td, values):
    """host t = C - 1 sizes the grid, the device value decides: same bits as the call with the exact host t"""
    args = (64, 4, 2, 2, 2, 100, 192, td, values, (13, 0))
    s = _make(*args)
    a = _run_one(s, backend, via_dev=True)
    _check_one(f"one-tdev{td}-{values}", s, a, backend)
    b = _run_one(s, backend)
    nsl = (s.P + 63) // 64 + (td + 63) // 64 + 1
    assert torch.equal(_bits(a.o), _bits(b.o))
    assert torch.equal(_bits(a.kc), _bits(b.kc)) and torch.equal(_bits(a.vct), _bits(b.vct))
    assert torch.equal(a.part_o.cpu()[:, :nsl].view(torch.int32), b.part_o.cpu()[:, :nsl].view(torch.int32))
    assert torch.equal(a.part_ml.cpu()[:, :nsl].view(torch.int32), b.part_ml.cpu()[:, :nsl].view(torch.int32))


LAYOUT_GEOMS = [("strided",), ("vt_wide",), ("ldo",), ("cp_wide",), ("table",), ("all",)]


@pytest.mark.parametrize("what,values", _with_adv(LAYOUT_GEOMS))
def test_one_layouts(backend, what, values):
    kw = {"strided": dict(strided=True), "vt_wide": dict(vt_extra=8), "ldo": dict(ldo_extra=8), "cp_wide": dict(cp_extra=8),
          "table": dict(use_rows=False), "all": dict(strided=True, vt_extra=16, ldo_extra=8, cp_extra=8, use_rows=False)}[what]
    _one(backend, f"layout-{what}", 128, 4, 2, 2, 3, 150, 128, 65, values, pad=(13, 0), **kw)


@pytest.mark.parametrize("what", ["nslot257", "nslot_short", "t_is_C"])
def test_one_refusals(backend, what):
    """an error code and no launch: nothing is written (the buffers are allocated for the larger of the two slot counts)"""
    s = _make(64, 2, 1, 1, 2, 70, 64, 1)
    need = 2 + 1 + 1
    kw = {"nslot257": dict(nslot=257), "nslot_short": dict(nslot=need, nslot_arg=need - 1), "t_is_C": dict(host_t=64)}[what]
    o_ = _Step()
    with pytest.raises(_lib.KernelError) as e:
        _run_one(s, backend, out=o_, **kw)
    assert e.value.status == _lib.BRA_ERR_ARG
    assert bool(torch.isnan(o_.part_o.cpu()).all()) and bool(torch.isnan(o_.part_ml.cpu()).all()) and bool((o_.o.cpu().float() == 3.0).all())
    assert torch.equal(_bits(o_.kc), _bits(o_.kc0)) and torch.equal(_bits(o_.vct), _bits(o_.vct0))


# ----------------------------------------------------------------------------- first generation: bra_dec_attn_both + merge
def _run_both(s, dev, via_dev=False, use_mask=True, use_rows=True, three_launches=False):
    """bra_dec_attn_both + merge; three_launches: bra_dec_attn_shared, bra_dec_attn_partial behind the prompt chunks (chunk_off = npc), merge"""
    B, Hq, Hkv, hd, P, C, t = s.B, s.Hq, s.Hkv, s.hd, s.P, s.C, s.t
    Nq, Nkv = Hq * hd, Hkv * hd
    o_ = _Step()
    (kp, sr, sh, ss), (vtp, vsr, vsh, vsd) = _prompt_buffers(s, dev)
    kc = torch.full((B, Hkv, C, hd), float("nan"), dtype=BF)           # rows > t are never read: indices clamp to t
    vc = torch.full((B, Hkv, C, hd), float("nan"), dtype=BF)
    kc[:, :, :t], vc[:, :, :t] = s.kold, s.vold
    kc[:, :, t], vc[:, :, t] = 5.5, 5.5                                # row t before the append: a zero-weight VALU operand, finite
    o_.kc0, o_.vc0 = kc.clone(), vc.clone()
    npc = (P + 63) // 64
    th = C - 1 if via_dev else t
    ntot_host, o_.ntot = npc + (th + 64) // 64, npc + (t + 64) // 64
    o_.part_o = torch.full((B * Hq * ntot_host + 2, hd), float("nan"), dtype=F32, device=dev)
    o_.part_ml = torch.full((B * Hq * ntot_host + 2, 2), float("nan"), dtype=F32, device=dev)
    o_.o = torch.full((B + 1, Nq), 3.0, dtype=BF, device=dev)
    rope_rows = torch.cat([s.cos[s.pos.long()], s.sin[s.pos.long()]], -1).contiguous().to(dev) if use_rows else None
    t_dev = torch.tensor([t], dtype=torch.int32, device=dev) if via_dev else None
    o_.kc, o_.vc = kc.to(dev), vc.to(dev)
    keep = (s.qkv.to(dev), s.qw.to(dev), s.kw.to(dev), s.cos.to(dev), s.sin.to(dev), s.pos.to(dev), s.pmask.to(dev))
    lib = _lib.get_lib()
    st = current_stream(keep[0])
    if three_launches:                             # (these two entry points take no rope rows: the position table)
        lib.call("bra_dec_attn_shared", keep[0], Nq + 2 * Nkv, keep[1], keep[3], keep[4], keep[5], kp, sr, sh, ss, vtp, vsr, vsh, vsd,
                 keep[6] if use_mask else None, o_.part_o, o_.part_ml, s.R, s.copies, Hq, Hkv, hd, P, ntot_host, EPS, s.scale, t_dev, st)
        lib.call("bra_dec_attn_partial", keep[0], Nq + 2 * Nkv, keep[1], keep[2], keep[3], keep[4], keep[5], o_.kc, o_.vc, None, o_.part_o, o_.part_ml,
                 B, Hq, Hkv, hd, C, th, EPS, s.scale, npc, ntot_host, t_dev, st)
    else:
        lib.call("bra_dec_attn_both", keep[0], Nq + 2 * Nkv, keep[1], keep[2], keep[3], keep[4], keep[5], kp, sr, sh, ss, vtp, vsr, vsh, vsd,
                 keep[6] if use_mask else None, o_.kc, o_.vc, o_.part_o, o_.part_ml, s.R, s.copies, Hq, Hkv, hd, P, C, th, EPS, s.scale, t_dev,
                 rope_rows, st)
    lib.call("bra_attn_decode_merge", o_.part_o, o_.part_ml, o_.o, B, Hq, hd, ntot_host, t_dev, npc, current_stream(keep[0]))
    if dev.type == "cuda":
        torch.cuda.synchronize()
    return o_


def _check_cache_rows(name, s, kc, vc, kc0, vc0, t):
    """row-major caches [B, Hkv, S, hd]: row t = the new k / v, everything else unchanged"""
    kc, vc = kc.cpu(), vc.cpu()
    _assert_appended_k(name, kc[:, :, t], s.k_pre, s.k_near)
    assert torch.equal(_bits(vc[:, :, t]), _bits(s.vn)), (name, "appended V row")
    kc0, vc0 = kc0.clone(), vc0.clone()
    kc0[:, :, t], vc0[:, :, t] = kc[:, :, t], vc[:, :, t]
    assert torch.equal(_bits(kc), _bits(kc0)) and torch.equal(_bits(vc), _bits(vc0)), (name, "cache elements besides the append changed")


def _check_both(name, s, o_, backend):
    B, Hq, hd = s.B, s.Hq, s.hd
    o = o_.o.cpu()
    assert bool((o[B:].float() == 3.0).all()), (name, "rows past B written")
    _check_rows(name, "attn", backend, o[:B].to(F64).reshape(B * Hq, hd), _step_rows(s, False), 3 * U)
    _check_cache_rows(name, s, o_.kc, o_.vc, o_.kc0, o_.vc0, s.t)
    n = B * Hq * o_.ntot
    po, pml = o_.part_o.cpu(), o_.part_ml.cpu()
    assert bool(torch.isfinite(po[:n]).all()) and bool(torch.isfinite(pml[:n]).all()), (name, "a slot the merge reads is not finite")
    assert bool(torch.isnan(po[n:]).all()) and bool(torch.isnan(pml[n:]).all()), (name, "a slot past the last chunk was written")


# (hd, Hq, Hkv, R, copies, P, C, t, pad of prompt 0, device-side t)
BOTH_GEOMS = [(128, 2, 2, 2, 3, 100, 128, t, 13, False) for t in (0, 63, 64, 65)] + [
    (128, 4, 2, 2, 2, 200, 128, 70, 70, False), (128, 4, 2, 2, 2, 200, 128, 5, 128, False),
    (64, 8, 2, 2, 2, 129, 128, 64, 64, False), (128, 2, 2, 1, 8, 65, 128, 127, 0, False), (128, 4, 2, 1, 8, 65, 128, 1, 0, False),
    (128, 4, 2, 2, 2, 100, 192, 0, 13, True), (64, 8, 2, 2, 2, 100, 192, 70, 13, True), (128, 2, 2, 2, 3, 100, 192, 64, 0, True)]


@pytest.mark.parametrize("hd,Hq,Hkv,R,copies,P,C,t,pad,via_dev,values", _with_adv(BOTH_GEOMS))
def test_both_and_merge(backend, hd, Hq, Hkv, R, copies, P, C, t, pad, via_dev, values):
    s = _make(hd, Hq, Hkv, R, copies, P, C, t, values, (pad, 0)[:R])
    name = f"both-hd{hd}-{Hq}x{Hkv}-R{R}c{copies}-P{P}-t{t}-pad{pad}-{'dev' if via_dev else 'host'}-{values}"
    a = _run_both(s, backend, via_dev=via_dev, use_rows=(t % 2 == 0))
    _check_both(name, s, a, backend)
    if via_dev:
        b = _run_both(s, backend)
        assert torch.equal(_bits(a.o), _bits(b.o)) and torch.equal(_bits(a.kc), _bits(b.kc)) and torch.equal(_bits(a.vc), _bits(b.vc))


@pytest.mark.parametrize("hd,Hq,Hkv,R,copies,P,C,t,pad,via_dev,values", [g for g in _with_adv(BOTH_GEOMS) if g[7] in (0, 64, 70)])
def test_shared_partial_and_merge(backend, hd, Hq, Hkv, R, copies, P, C, t, pad, via_dev, values):
    """the same step as three launches: the prompt part and the completion part through their own entry points, the completion
    part's chunks behind the prompt's (chunk_off = npc; one wave per kv-head there, one per q-head in bra_dec_attn_both)"""
    s = _make(hd, Hq, Hkv, R, copies, P, C, t, values, (pad, 0)[:R])
    name = f"three-hd{hd}-{Hq}x{Hkv}-R{R}c{copies}-P{P}-t{t}-pad{pad}-{'dev' if via_dev else 'host'}-{values}"
    a = _run_both(s, backend, via_dev=via_dev, use_rows=False, three_launches=True)
    _check_both(name, s, a, backend)


@pytest.mark.parametrize("values", ["rand", "dom_new", "dom_prompt", "mixed_v"])
def test_both_past_256_chunks(backend, values):
    """npc + ncc = 258: the merge's branch for more than 256 chunks, through the full path (the new key sits in chunk 257)"""
    s = _make(64, 1, 1, 1, 1, 64 * 256 - 3, 128, 70, values)
    o_ = _run_both(s, backend)
    assert o_.ntot == 258
    _check_both(f"both-258-{values}", s, o_, backend)


def test_both_refuses_17_rows(backend):
    s = _make(64, 1, 1, 1, 17, 70, 64, 1)
    with pytest.raises(_lib.KernelError) as e:
        _run_both(s, backend)
    assert e.value.status == _lib.BRA_ERR_UNSUPPORTED


# ----------------------------------------------------------------------------- the non-shared fused step: bra_dec_attn_partial + merge
# (hd, Hq, Hkv, B, Smax, cur_len, device-side cur_len)
PARTIAL_GEOMS = [(128, 4, 2, 3, 320, n, False) for n in (0, 63, 64, 255, 256)] + [
    (32, 4, 1, 3, 320, 64, False), (32, 2, 2, 2, 320, 255, True), (64, 2, 1, 3, 320, 63, True), (128, 2, 2, 2, 320, 256, True), (64, 4, 1, 2, 320, 0, True)]


def _make_partial(hd, Hq, Hkv, B, Smax, n, values):
    """the step's tensors with the `n` cached keys as one per-sequence `prompt` (R = B, copies = 1): row 0 left-padded, row 1 not"""
    s = _make(hd, Hq, Hkv, B, 1, max(n, 1), Smax, 0, values, ((min(13, n - 1),) if n > 1 else ()))
    if n == 0:                                     # no cached key at all: the one prompt key of _make is masked out of the reference
        s.pmask[:] = 0
    return s


@pytest.mark.parametrize("hd,Hq,Hkv,B,Smax,n,via_dev,values", _with_adv(PARTIAL_GEOMS))
def test_partial_and_merge(backend, hd, Hq, Hkv, B, Smax, n, via_dev, values):
    dev = backend
    s = _make_partial(hd, Hq, Hkv, B, Smax, n, values)
    name = f"partial-hd{hd}-{Hq}x{Hkv}-B{B}-len{n}-{'dev' if via_dev else 'host'}-{values}"
    Nq, Nkv = Hq * hd, Hkv * hd
    kc = torch.full((B, Hkv, Smax, hd), float("nan"), dtype=BF)
    vc = torch.full((B, Hkv, Smax, hd), float("nan"), dtype=BF)
    kmask = torch.zeros(B, Smax, dtype=torch.uint8)                    # position n (the new key) stays 0: the kernel admits it by index
    if n:
        kc[:, :, :n], vc[:, :, :n], kmask[:, :n] = s.kp, s.vp, s.pmask
    kc[:, :, n], vc[:, :, n] = 5.5, 5.5                                # row n before the append: a zero-weight VALU operand, finite
    kc0, vc0 = kc.clone(), vc.clone()
    host_n = Smax - 1 if via_dev else n
    nch_host, nch = (host_n + 64) // 64, (n + 64) // 64
    part_o = torch.full((B * Hq * nch_host + 2, hd), float("nan"), dtype=F32, device=dev)
    part_ml = torch.full((B * Hq * nch_host + 2, 2), float("nan"), dtype=F32, device=dev)
    o = torch.full((B + 1, Nq), 3.0, dtype=BF, device=dev)
    t_dev = torch.tensor([n], dtype=torch.int32, device=dev) if via_dev else None
    kcd, vcd = kc.to(dev), vc.to(dev)
    keep = (s.qkv.to(dev), s.qw.to(dev), s.kw.to(dev), s.cos.to(dev), s.sin.to(dev), s.pos.to(dev), kmask.to(dev))
    lib = _lib.get_lib()
    lib.call("bra_dec_attn_partial", keep[0], Nq + 2 * Nkv, keep[1], keep[2], keep[3], keep[4], keep[5], kcd, vcd, keep[6], part_o, part_ml,
             B, Hq, Hkv, hd, Smax, host_n, EPS, s.scale, 0, 0, t_dev, current_stream(keep[0]))
    lib.call("bra_attn_decode_merge", part_o, part_ml, o, B, Hq, hd, nch_host, t_dev, 0, current_stream(keep[0]))
    if dev.type == "cuda":
        torch.cuda.synchronize()
    oc = o.cpu()
    assert bool((oc[B:].float() == 3.0).all())
    rows = [(lab, ref, A, 0.0) for lab, ref, A, _ in _step_rows(s, False)]          # no key goes through an MFMA
    _check_rows(name, "attn", backend, oc[:B].to(F64).reshape(B * Hq, hd), rows, 2 * U)
    _check_cache_rows(name, s, kcd, vcd, kc0, vc0, n)
    m = B * Hq * nch
    assert bool(torch.isfinite(part_o.cpu()[:m]).all()) and bool(torch.isnan(part_o.cpu()[m:]).all()) and bool(torch.isnan(part_ml.cpu()[m:]).all())


# ----------------------------------------------------------------------------- ops.attn_decode (128-key chunks, q given)
@pytest.mark.parametrize("hd,Hq,Hkv,L,values", [(hd, Hq, Hkv, L, v) for (hd, Hq, Hkv) in ((128, 4, 2), (64, 2, 2), (32, 4, 1))
                                                 for L in (1, 127, 128, 129) for v in ("rand", "mixed_v")]
                         + [(32, 2, 1, 128 * 256 + 1, "rand"), (32, 2, 1, 128 * 256 + 1, "mixed_v")])
def test_attn_decode_rows(backend, hd, Hq, Hkv, L, values):
    """(the last two: 257 chunks — bra_attn_decode's own merge launch past 256 chunks; the last key carries the weight)"""
    dev = backend
    B, Smax = (2, L + 7) if L > 1000 else (3, 320)
    g = torch.Generator().manual_seed(L + hd)
    q = torch.randn(B, Hq, hd, generator=g).to(BF)
    kc, vc = torch.randn(B, Hkv, Smax, hd, generator=g), torch.randn(B, Hkv, Smax, hd, generator=g)
    if values == "mixed_v":
        vc *= (2.0 ** ((torch.arange(Smax) % 13) - 6.0))[:, None]
    if L > 1000:                                   # the newest key dominates: it lives in the chunk past the 256th
        kc[:, :, L - 1] = 12.0 * q.float().view(B, Hkv, -1, hd)[:, :, 0] / hd ** 0.5
    kc, vc = kc.to(BF), vc.to(BF)
    kc[:, :, L:], vc[:, :, L:] = float("nan"), float("nan")
    kmask = torch.ones(B, Smax, dtype=torch.uint8)
    kmask[1, :min(11, L - 1)] = 0
    nch = (L + 127) // 128
    ws = (torch.full((B * Hq * nch + 2, hd), float("nan"), dtype=F32, device=dev), torch.full((B * Hq * nch + 2, 2), float("nan"), dtype=F32, device=dev),
          torch.full((B + 1, Hq * hd), 3.0, dtype=BF, device=dev))
    o = ops.attn_decode(q.to(dev), kc.to(dev), vc.to(dev), kmask.to(dev), L, hd ** -0.5, ws=ws).cpu()
    assert bool((o[B:].float() == 3.0).all()) and bool(torch.isnan(ws[0].cpu()[B * Hq * nch:]).all())
    rows = []
    none = torch.zeros(L, dtype=torch.bool)
    for b in range(B):
        for hq in range(Hq):
            h = hq // (Hq // Hkv)
            ref, A, _ = _row_ref(q[b, hq].to(F64), kc[b, h, :L].to(F64), vc[b, h, :L].to(F64), kmask[b, :L].bool(), none, hd ** -0.5)
            rows.append(((b, hq), ref, A, 0.0))
    _check_rows(f"attn_decode-hd{hd}-{Hq}x{Hkv}-L{L}-{values}", "attn", backend, o[:B].to(F64).reshape(B * Hq, hd), rows, 2 * U)


# ----------------------------------------------------------------------------- the merge kernel alone
MERGE_COUNTS = [1, 47, 48, 49, 56, 57, 64, 65, 255, 256, 257, 300, 513]


def _merge_partials(n, hd, B, Hq, seed, dominant):
    g = torch.Generator().manual_seed(seed)
    m = 4.0 * torch.randn(B, Hq, n, generator=g)
    l = 1.0 + 63.0 * torch.rand(B, Hq, n, generator=g)
    O = torch.randn(B, Hq, n, hd, generator=g) * l[..., None]
    empty = torch.rand(B, Hq, n, generator=g) < 0.2
    empty[..., dominant] = False
    empty[0, 0] = False                            # one row without an empty slot
    m[empty], l[empty] = NEG, 0.0
    O[empty] = 777.0                               # what an empty slot holds is finite and must get weight 0
    m[..., dominant] += 40.0
    if n > 1:
        m[-1, -1, dominant] -= 40.0                # ... and one row without a dominant slot
    return m.to(F32), l.to(F32), O.to(F32)


@pytest.mark.parametrize("n,hd,via_dev", [(n, hd, v) for hd in (32, 64, 128) for n in MERGE_COUNTS for v in (False, True) if not (v and n < 2)])
def test_merge_alone(backend, n, hd, via_dev):
    """bra_attn_decode_merge on synthetic (max, sum, O) partials (max in log2 units) against the exact float64 merge; the dominant slot
    is the last one or the middle one, so that every 64-slot range carries the weight once"""
    dev = backend
    B, Hq = 2, 3
    dominant = n - 1 if (n + hd // 32) % 2 else n // 2
    m, l, O = _merge_partials(n, hd, B, Hq, 1000 * n + hd, dominant)
    part_ml = torch.full((B * Hq * n + 3, 2), float("nan"), dtype=F32)
    part_o = torch.full((B * Hq * n + 3, hd), float("nan"), dtype=F32)
    part_ml[:B * Hq * n] = torch.stack([m, l], -1).reshape(-1, 2)
    part_o[:B * Hq * n] = O.reshape(-1, hd)
    o = torch.full((B + 1, Hq * hd), 3.0, dtype=BF, device=dev)
    part_ml, part_o = part_ml.to(dev), part_o.to(dev)
    if via_dev:                                    # n = npc + (t + 64) / 64 on the device; the host count is another (larger) one
        ncc = min(3, n - 1)
        npc, t = n - ncc, 64 * ncc - 7
        t_dev = torch.tensor([t], dtype=torch.int32, device=dev)
        args = (n + 5, t_dev, npc)
    else:
        args = (n, None, 0)
    _lib.get_lib().call("bra_attn_decode_merge", part_o, part_ml, o, B, Hq, hd, args[0], args[1], args[2], current_stream(o))
    if dev.type == "cuda":
        torch.cuda.synchronize()
    oc = o.cpu()
    assert bool((oc[B:].float() == 3.0).all())
    md, ld, Od = m.to(F64), l.to(F64), O.to(F64)
    w = torch.exp2(md - md.max(-1, keepdim=True).values)
    w = torch.where(ld > 0, w, torch.zeros_like(w))
    L = (w * ld).sum(-1)
    ref = (w[..., None] * Od).sum(2) / L[..., None]
    A = (w[..., None] * Od.abs()).sum(2) / L[..., None]
    rows = [((b, hq), ref[b, hq], A[b, hq], 0.0) for b in range(B) for hq in range(Hq)]
    _check_rows(f"merge-n{n}-hd{hd}-{'dev' if via_dev else 'host'}", "merge", backend, oc[:B].to(F64).reshape(B * Hq, hd), rows, 2 * U)


# ----------------------------------------------------------------------------- the adversarial sets themselves (CPU)
@pytest.mark.parametrize("values", ADV)
@pytest.mark.parametrize("geom", [(128, 4, 2, 2, 2, 200, 128, 70, (70, 0)), (64, 2, 1, 1, 2, 1, 64, 0, ()), (128, 1, 1, 1, 1, 64 * 127 - 5, 64, 1, ())])
def test_adv_reference_is_finite(values, geom):
    s = _make(*geom[:8], values, geom[8])
    top = 0.0
    for label, ref, A, delta in _step_rows(s, True):
        assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(A).all()) and bool((A > 0).all()) and math.isfinite(delta), (values, label)
    if values in ("dom_prompt", "dom_new", "underflow") and s.P > 4:
        # the dominant key does dominate: its probability is above 0.99 in at least one row
        for b in range(s.B):
            for hq in range(0, s.Hq, s.G):
                K = torch.cat([s.kp[b // s.copies, hq // s.G].to(F64), s.kold[b, hq // s.G].to(F64), s.kn[b, hq // s.G][None]], 0)
                sc = s.scale * (K @ s.qn[b, hq])
                sc[:s.P][~s.pmask[b // s.copies].bool()] = -math.inf
                top = max(top, float(torch.softmax(sc, 0).max()))
        assert top > 0.99, (values, top)
