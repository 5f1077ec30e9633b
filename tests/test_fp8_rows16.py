"""fp8 (OCP e4m3) rollout weights at 9 .. 16 rows and in mixed fp8 / bf16 layers: bra_dec_pack_weights_fp8_rows, bra_dec_gemm2_fp8_rows
(k_decgemm.hip: dec_gemm2_kernel<.., WIDE = 1, .., F8 = 1>), the per-projection layer record of the step driver (k_decode.hip) and
generation.rollout_weights.  Helpers, value sets and allowances are those of tests/test_decode_proj_rowwise.py (element by element
against float64) and tests/test_fp8_rollout.py (the fp32 statement over the codes and scales read back; the end-to-end oracle).

  packer   the rows = 16 image, un-permuted with 16-column tiles, holds the codes and scales of the rows = 8 image bit for bit.  Where the
           8-row class has no image of the same projection (its diagonal tiles start at K = 1024, its 16-column tiles end at K = 3072)
           the 8-row image of the same matrix in the other tile mode is the comparand — the same quantiser, another order.
  exact    x integers |v| <= 4, W integers in [-7, 7] with a 7 in every row: scale 2^-6 and codes 64 W asserted, every partial sum below
           4 * 448 * 6144 < 2^24, so fp32 outputs equal the float64 product, bf16 outputs rnd(acc) and rnd(rnd(acc) + res), bit for bit, at
           the eight (waves, chunks) forms K = 512 .. 6144 and M = 9, 13, 16.  SwiGLU: test_decode_proj_rowwise's rule (bit for bit against
           the float64 twin, one ulp only where silu(g) is boundary-near) on inputs that keep that rule's premises under the exact fp8 rule:
           x = +-2^j equal in column pairs, every weight row one (7 s, s) pair — 8 s x, a power of two, and the row maximum 7 — gate rows
           three more entries +-{1, 2, 4}.
  probe    the folded statistics, fp32 output, x one-hot: W entries +-2^j with one 7 per row off the probed columns (scale 2^-6: both
           epilogue factors but rstd are powers of two), so out / W = the device's rstd of that row, held to tau_rstd u.
  random   test_fp8_rollout's criterion and bounds; row r of an M = 16 launch equals row r of an M = 9 launch bit for bit.
  end to end (GPU): the criterion of test_rollout_over_fp8_weights_against_the_oracle_with_the_same_fake_quantised_weights.

Emulator cases above 4.3e6 weight elements are skipped; each names the smaller case of the same form that runs there."""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bioreason_amd import ops, _lib                                                          # noqa: E402
from test_gemm_family_rowwise import _bf, _assert_bits, _ties, _Window, U32                  # noqa: E402
from test_decode_proj_rowwise import (_fp8_inputs, _check_ss, _mirror, _pow2, _swiglu_twin, _assert_swiglu, _tau_rstd, _probe_stats,   # noqa: E402
                                      EPS, EMU_MAX, UNSUPPORTED)
from test_layer_glue_rowwise import NEAR_CAP                                                 # noqa: E402
from test_fp8_rollout import unpack_fp8, unpack_fp8_fast, rel, rnd                           # noqa: E402

BF, F32, F64, F8 = torch.bfloat16, torch.float32, torch.float64, torch.float8_e4m3fn
# K of the eight single-round (waves, chunks) forms of the 16-row class
FORMS = {512: (4, 4), 1024: (4, 8), 1536: (4, 12), 2048: (8, 8), 2560: (8, 10), 3072: (8, 12), 4096: (16, 8), 6144: (16, 12)}


def _emu_skip(dev, N, K, smaller):
    if dev.type == "cpu" and N * K > EMU_MAX:
        pytest.skip(f"emulator: {N} x {K} weights; the same form at {smaller}")


def _diag8(N, K, act, f32):
    """8-column (diagonal) tiles of the 8-row class"""
    return (not act) and (not f32) and N % 8 == 0 and K % 64 == 0 and (N + 15) // 16 < 256 and N // 8 <= 256


def _call(x, q, sc, win, M, N, K, *, ss_in=None, nss=0, res=None, sw=None, act=False, f32=False, image_rows=16, entry="bra_dec_gemm2_fp8_rows"):
    args = [x, x.stride(0), ss_in, nss, EPS, q, sc, res, res.stride(0) if res is not None else 0, win.win, win.win.stride(0),
            sw.win if sw else None, sw.win.stride(0) if sw else 0, M, N, K, int(act), int(f32), int(ss_in is not None)]
    if entry == "bra_dec_gemm2_fp8_rows":
        args.append(image_rows)
    return _lib.get_lib().call_rc(entry, *args, _lib.current_stream(x))


# ----------------------------------------------------------------------------- 1: the packer
def test_the_mirror_names_the_eight_forms():
    for K, (nw, nl) in FORMS.items():
        f = _mirror(16, 48, K, "f32", False, 1)["form"]
        assert (f.rows, f.mode, f.nw, f.nl, f.kind) == (16, 0, nw, nl, "fast"), (K, f)


@pytest.mark.parametrize("N,act,f32", [(48, 0, 0), (96, 1, 0), (80, 0, 1)])
@pytest.mark.parametrize("K", [512, 2048, 6144])
def test_rows16_image_holds_the_codes_and_scales_of_the_rows8_image(backend, K, N, act, f32):
    W = rnd(N, K, dev=backend, scale=0.05, seed=K + N)
    W[1] = 0                                                                     # an all-zero row: scale 1, codes 0
    nw = (1.0 + 0.1 * torch.randn(K, generator=torch.Generator().manual_seed(2))).to(BF).to(backend)
    for norm in (None, nw):
        got = ops.dec_pack_weights_fp8(W, act=bool(act), out_f32=bool(f32), norm_w=norm, rows=16)
        assert got is not None, (N, K)
        q16, s16 = got
        assert q16.dtype == torch.uint8 and tuple(q16.shape) == (N, K) and tuple(s16.shape) == (N,)
        ref = ops.dec_pack_weights_fp8(W, act=bool(act), out_f32=bool(f32), norm_w=norm)            # rows = 8
        diag = _diag8(N, K, act, f32)
        same_flags = ref is not None
        assert same_flags == (not (diag and K == 512) and not (not diag and K == 6144))
        if ref is None:         # the 8-row class streams K = 512 on 16-column tiles only and K = 6144 on diagonal tiles only
            diag = K == 6144
            ref = ops.dec_pack_weights_fp8(W, out_f32=not diag, norm_w=norm)
        q8, s8 = ref
        codes16 = unpack_fp8_fast(q16, N, K, False)
        assert torch.equal(codes16, unpack_fp8_fast(q8, N, K, diag))
        assert torch.equal(s16.cpu().view(torch.int32), s8.cpu().view(torch.int32))
        assert (codes16[1] == 0).all() and s16[1].item() == 1.0 and int(codes16.view(F8).float().abs().max()) == 448
        if K == 512:
            assert torch.equal(codes16, unpack_fp8(q16, N, K, False))            # the readable statement of the order
        if f32 and same_flags:
            assert torch.equal(q16.cpu(), q8.cpu())                              # fp32-output projections: one image for both row classes
        ops8 = ops.dec_pack_weights_fp8(W, act=bool(act), out_f32=bool(f32), norm_w=norm, rows=8)
        assert (ops8 is None) == (not same_flags) and (ops8 is None or torch.equal(ops8[0].cpu(), ref[0].cpu()))


def test_rows16_packer_refuses_what_the_kernel_cannot_stream(backend):
    lib = _lib.get_lib()
    for rows in (16, 8):
        assert ops.dec_pack_weights_fp8(rnd(64, 9728, dev=backend, scale=0.05), rows=rows) is None      # two register rounds
        assert ops.dec_pack_weights_fp8(rnd(64, 256, dev=backend), rows=rows) is None                   # less than one round of 4 waves
        assert ops.dec_pack_weights_fp8(rnd(64, 96, dev=backend), rows=rows) is None                    # an odd number of k-steps
        assert ops.dec_pack_weights_fp8(rnd(40, 2048, dev=backend), rows=rows, out_f32=True) is None    # not a tile multiple
    assert ops.dec_pack_weights_fp8(rnd(64, 9728, dev=backend, scale=0.05)) is None                     # (the default is rows = 8)
    assert ops.dec_pack_weights_fp8(rnd(48, 5120, dev=backend), rows=16) is None                        # 16 waves x 10 steps: no such form
    assert ops.dec_pack_weights_fp8(rnd(48, 4096, dev=backend), rows=16) is not None                    # 16 x 8 ...
    assert ops.dec_pack_weights_fp8(rnd(48, 4096, dev=backend), out_f32=True) is None                   # ... which 8 rows do not have
    W = rnd(48, 2048, dev=backend)
    q, sc = torch.zeros(48, 2048, dtype=torch.uint8, device=backend), torch.zeros(48, device=backend)
    for rows in (0, 17, -1):
        with pytest.raises(_lib.KernelError) as e:
            lib.call("bra_dec_pack_weights_fp8_rows", W, 2048, 48, 2048, 0, 0, None, rows, q, sc, _lib.current_stream(W))
        assert e.value.status == _lib.BRA_ERR_ARG
    assert int(q.sum()) == 0 and float(sc.sum()) == 0.0


# ----------------------------------------------------------------------------- 2: the exact set
def _pack_exact(dev, d, N, K, act=False, f32=False):
    got = ops.dec_pack_weights_fp8(d["W"].to(dev), act=act, out_f32=f32, rows=16)
    assert got is not None
    q, sc = got
    assert (sc.cpu() == 2.0 ** -6).all()
    assert torch.equal(unpack_fp8_fast(q, N, K, False).view(F8).to(F64), 64 * d["W"].to(F64))
    return q, sc


def _exact_case(dev, M, N, K, epi, tally):
    f32 = epi in ("f32", "f32max")
    m = _mirror(M, N, K, epi, False, 1)
    assert (m["form"].rows, m["form"].kind, (m["form"].nw, m["form"].nl)) == (16, "fast", FORMS[K])
    name = f"fp8-16r-{m['form'].nw}x{m['form'].nl}-{epi}-{M}x{N}x{K}"
    d = _fp8_inputs(M, N, K, "exact")
    q, sc = _pack_exact(dev, d, N, K, f32=f32)
    x = d["x"].to(dev)
    win = _Window(M, N, F32 if f32 else BF, dev, "direct" if M % 2 else "lds")
    res = d["res"].to(dev) if epi == "res" else None
    sw = _Window(M, m["ntiles"], F32, dev, "direct") if epi in ("res", "f32max") else None
    rc = _call(x, q, sc, win, M, N, K, res=res, sw=sw, f32=f32)
    assert rc == 0, (name, rc)
    got = win.result(name)                                                       # (rows >= M and everything around the window: untouched)
    acc, R = d["x"].to(F64) @ d["W"].to(F64).T, d["res"].to(F64)
    assert (d["x"].to(F64).abs() @ (64 * d["W"].to(F64)).abs().T).max() < 2 ** 24
    want = acc.to(F32) if f32 else ((_bf(acc) + R).to(BF) if epi == "res" else acc.to(BF))
    if not f32:
        tally["ties"] = tally.get("ties", 0) + _ties(acc) + (_ties(_bf(acc) + R) if epi == "res" else 0)
    _assert_bits(name, got, want)
    if epi == "res":
        tally["ss_exact"] = tally.get("ss_exact", 0) + _check_ss(name, sw.result(name + " ss_out"), got, 16, m["ntiles"])
    if epi == "f32max":
        _assert_bits(name + " tile maxima", sw.result(name + " tile maxima"), got.view(M, m["ntiles"], 16).amax(-1))
    return m


def _act_inputs(M, K, attempt):
    """the SwiGLU set under the exact fp8 rule (module docstring) -> dict for _swiglu_twin"""
    N = 96
    g = torch.Generator().manual_seed(7919 * M + K + 31 * attempt)
    x = _pow2(g, (M, K // 2), -2, 0).repeat_interleave(2, dim=1)
    W = torch.zeros(N, K, dtype=F64)
    rows = torch.arange(N)
    gate = (rows % 16) < 8
    c = torch.randint(0, K // 2, (N,), generator=g)
    for _ in range(3):
        cc, v = torch.randint(0, K, (N,), generator=g), _pow2(g, (N,), 0, 2)
        put = gate & (cc // 2 != c)
        W[rows[put], cc[put]] = v[put]
    s = torch.randint(0, 2, (N,), generator=g).to(F64) * 2 - 1
    W[rows, 2 * c], W[rows, 2 * c + 1] = 7 * s, s
    return {"M": M, "N": N, "K": K, "x": x.to(BF), "W": W.to(BF), "nw": torch.ones(K, dtype=BF)}


def _act_case(dev, M, K):
    for attempt in range(8):
        d = _act_inputs(M, K, attempt)
        twin = _swiglu_twin(d, 0)
        if (twin[1] | twin[2]).float().mean().item() <= NEAR_CAP:
            break
    else:
        raise AssertionError(("no SwiGLU input set within the cap", M, K))
    N = 96
    q, sc = _pack_exact(dev, d, N, K, act=True)
    win = _Window(M, N // 2, BF, dev, "lds" if M % 2 else "direct")
    x = d["x"].to(dev)
    name = f"fp8-16r-act-{M}x{N}x{K}"
    assert _call(x, q, sc, win, M, N, K, act=True) == 0, name
    _assert_swiglu(name, win.result(name), twin)


@pytest.mark.parametrize("M", [9, 13, 16])
@pytest.mark.parametrize("K", list(FORMS))
def test_exact_every_form_every_epilogue(backend, K, M):
    """bra_dec_pack_weights_fp8_rows(rows = 16) + bra_dec_gemm2_fp8_rows(image_rows = 16), no norm: fp32 (+ tile maxima), bf16, residual +
    ss_out bit for bit, SwiGLU by its rule; rows >= M of every output keep the pattern they held"""
    tally = {}
    for epi in ("f32max", "f32", "bf16", "res"):
        _exact_case(backend, M, 48, K, epi, tally)
    _act_case(backend, M, K)
    assert tally["ss_exact"] > 0
    assert K < 1024 or tally["ties"] > 0, tally


@pytest.mark.parametrize("M,N,K,cap,hip_only", [(13, 8208, 512, 512, False), (16, 4112, 2048, 256, True)])
def test_exact_later_tiles_of_a_workgroup(backend, M, N, K, cap, hip_only):
    """more tiles than the grid cap: weights and scales ping-pong, the epilogue wave rotates, the residual is loaded in the epilogue"""
    if hip_only:
        _emu_skip(backend, N, K, "K = 512, N = 8208 (the 512-workgroup cap of four waves)")
    tally = {}
    for epi in ("res", "f32max"):
        m = _exact_case(backend, M, N, K, epi, tally)
        assert m["later"] and m["grid"] == cap
    assert tally["ties"] > 0 and tally["ss_exact"] > 0


# ----------------------------------------------------------------------------- 3: the folded statistics, row by row
@pytest.mark.parametrize("K", [512, 4096])
@pytest.mark.parametrize("nss", [32, 256])
@pytest.mark.parametrize("M", [9, 16])
def test_folded_statistics_per_row(backend, M, nss, K):
    """out[m, n] = rstd_m scale[n] code[n, k_m] with scale = 2^-6 and code = 64 W a power of two: out / W is the device's rstd of row m, against
    rsqrt(sum of ALL nss columns of row m / K + eps) within tau_rstd u; rows >= M of ss_in hold 1e30 and must not reach any row"""
    N = 48
    ss, rstd = _probe_stats(M, nss, K)
    g = torch.Generator().manual_seed(M + nss + K)
    perm = torch.randperm(K, generator=g)
    km, k7 = perm[:M], perm[M:M + N]
    x = torch.zeros(M, K, dtype=F64)
    x[torch.arange(M), km] = 1.0
    W = _pow2(g, (N, K), -3, 2)
    W[torch.arange(N), k7] = 7.0
    dev = backend
    got = ops.dec_pack_weights_fp8(W.to(BF).to(dev), out_f32=True, norm_w=torch.ones(K, dtype=BF).to(dev), rows=16)
    assert got is not None
    q, sc = got
    assert (sc.cpu() == 2.0 ** -6).all() and torch.equal(unpack_fp8_fast(q, N, K, False).view(F8).to(F64), 64 * W)
    win = _Window(M, N, F32, dev)
    xd = x.to(BF).to(dev)
    assert _call(xd, q, sc, win, M, N, K, ss_in=ss.to(dev), nss=nss, f32=True) == 0
    out = win.result(f"fp8-probe-{M}-{nss}-{K}").to(F64)
    r = out / W[:, km].T
    err = (r - rstd[:, None]).abs() / rstd[:, None]
    assert (err <= _tau_rstd(nss) * U32).all(), (M, nss, K, "rows", sorted(set(torch.nonzero(err > _tau_rstd(nss) * U32)[:, 0].tolist())), err.max().item() / U32)


# ----------------------------------------------------------------------------- 4: random values
def _statement(xf, q, scale, N, K, folded, act, res):
    """test_fp8_rollout's fp32 statement over the codes and scales read back (16-column tiles)"""
    M = xf.shape[0]
    wq = unpack_fp8_fast(q, N, K, False).view(F8).float()
    y = (xf @ wq.T) * scale.cpu()[None, :]
    if folded:
        y = y * torch.rsqrt((xf * xf).mean(-1, keepdim=True) + 1e-6)
    if act:
        y = y.view(M, N // 16, 2, 8)
        y = (torch.nn.functional.silu(y[:, :, 0].to(BF).float()).to(BF).float() * y[:, :, 1].to(BF).float()).reshape(M, N // 2)
    if res is not None:
        y = y.to(BF).float() + res.float().cpu()
    return y


RANDOM = [(16, 4096, 2048, 0, 0, "16 x 64 x 2048"), (16, 64, 2048, 0, 0, None),
          (12, 2048, 6144, 0, 0, "12 x 64 x 6144"), (12, 64, 6144, 0, 0, None),
          (16, 12288, 2048, 1, 0, "16 x 96 x 2048 SwiGLU"), (16, 96, 2048, 1, 0, None),
          (9, 8208, 2048, 0, 1, "9 x 80 x 2048 fp32"), (9, 80, 2048, 0, 1, None)]


@pytest.mark.parametrize("M,N,K,act,f32,smaller", RANDOM)
def test_random_against_fp32_over_the_same_quantised_weights(backend, M, N, K, act, f32, smaller):
    if smaller:
        _emu_skip(backend, N, K, smaller)
    x16, W = rnd(16, K, dev=backend, seed=3), rnd(N, K, dev=backend, scale=0.05, seed=4)
    nw = (1.0 + 0.1 * torch.randn(K, generator=torch.Generator().manual_seed(5))).to(BF).to(backend)
    x = x16[:M].contiguous()
    xf = x.float().cpu()
    No = N // 2 if act else N
    # (1) norm folded: the qkv / gate-up / lm_head forms
    q, sc = ops.dec_pack_weights_fp8(W, act=bool(act), out_f32=bool(f32), norm_w=nw, rows=16)
    tm = torch.full((M, N // 16), -7.0, device=backend) if f32 else None
    got = ops.dec_gemm2_fp8(x, q, sc, ss_in=ops.row_sumsq(x, 256), act=bool(act), out_f32=bool(f32), tile_max=tm, image_rows=16)
    assert got is not None
    y = got[0]
    assert tuple(y.shape) == (M, No)
    e = rel(y, _statement(xf, q, sc, N, K, True, act, None))
    print(f"\n[fp8-rows16] {M}x{N}x{K} act {act} f32 {f32}: folded rel {e:.3e}")
    assert e < (2e-5 if f32 else 4e-3), e
    if f32:
        assert torch.equal(tm.cpu(), y.float().view(M, N // 16, 16).amax(-1).cpu())
    # row r of an M = 16 launch is row r of an M = 9 launch
    tm16 = torch.full((16, N // 16), -7.0, device=backend) if f32 else None
    tm9 = torch.full((9, N // 16), -7.0, device=backend) if f32 else None
    kw = dict(act=bool(act), out_f32=bool(f32), image_rows=16)
    y16 = ops.dec_gemm2_fp8(x16, q, sc, ss_in=ops.row_sumsq(x16, 256), tile_max=tm16, **kw)[0]
    x9 = x16[:9].contiguous()
    y9 = ops.dec_gemm2_fp8(x9, q, sc, ss_in=ops.row_sumsq(x9, 256), tile_max=tm9, **kw)[0]
    assert torch.equal(y16[:9].cpu().view(torch.int32 if f32 else torch.int16), y9.cpu().view(torch.int32 if f32 else torch.int16))
    if f32:
        assert torch.equal(tm16[:9].cpu(), tm9.cpu())
    # (2) no norm, residual + statistics: the o / down forms
    if not act and not f32:
        q2, sc2 = ops.dec_pack_weights_fp8(W, rows=16)
        r = rnd(M, N, dev=backend, seed=6)
        y2, s2 = ops.dec_gemm2_fp8(x, q2, sc2, res=r, want_ss=True, image_rows=16)
        e2 = rel(y2, _statement(xf, q2, sc2, N, K, False, False, r))
        print(f"[fp8-rows16] {M}x{N}x{K}: residual rel {e2:.3e}")
        assert e2 < 4e-3, e2
        assert tuple(s2.shape)[0] == 16 and rel(s2[:M].sum(1), (y2.float() ** 2).sum(1)) < 1e-2
        r16 = rnd(16, N, dev=backend, seed=6)
        a, sa = ops.dec_gemm2_fp8(x16, q2, sc2, res=r16, want_ss=True, image_rows=16)
        b, sb = ops.dec_gemm2_fp8(x9, q2, sc2, res=r16[:9].contiguous(), want_ss=True, image_rows=16)
        assert torch.equal(a[:9].cpu().view(torch.int16), b.cpu().view(torch.int16)) and torch.equal(sa[:9].cpu(), sb[:9].cpu())


# ----------------------------------------------------------------------------- 5: the old entry points and the pairing of image and rows
def test_old_entry_points_and_row_classes(backend):
    x12 = rnd(12, 2048, dev=backend)
    W = rnd(64, 2048, dev=backend, scale=0.05)
    q, sc = ops.dec_pack_weights_fp8(W)
    assert ops.dec_gemm2_fp8(x12, q, sc) is None                                  # the defaults: 8-row image, more than 8 rows
    q16, sc16 = ops.dec_pack_weights_fp8(W, rows=16)
    x8 = x12[:8].contiguous()
    assert ops.dec_gemm2_fp8(x8, q16, sc16, image_rows=16) is None                # a 16-row image streams against 9 .. 16 rows only
    assert ops.dec_gemm2_fp8(x12, q16, sc16, image_rows=12) is None               # no such class
    assert ops.dec_gemm2_fp8(rnd(17, 2048, dev=backend), q16, sc16, image_rows=16) is None
    assert ops.dec_gemm2_fp8(x12, q16, sc16, image_rows=16) is not None
    # bra_dec_gemm2_fp8 itself at M = 12: refused, nothing written
    for entry, extra in (("bra_dec_gemm2_fp8", {}), ("bra_dec_gemm2_fp8_rows", {"image_rows": 8})):
        win = _Window(12, 64, BF, backend)
        sw = _Window(12, 32, F32, backend, "direct")
        assert _call(x12, q, sc, win, 12, 64, 2048, res=rnd(12, 64, dev=backend), sw=sw, entry=entry, **extra) == UNSUPPORTED
        win.result(entry)
        sw.result(entry + " ss_out")
        assert torch.equal(win.buf.cpu(), win.before) and torch.equal(sw.buf.cpu(), sw.before)
    # the two names of the 8-row call give the same bits
    a, _ = ops.dec_gemm2_fp8(x8, q, sc)
    win = _Window(8, 64, BF, backend)
    assert _call(x8, q, sc, win, 8, 64, 2048, entry="bra_dec_gemm2_fp8") == 0
    assert torch.equal(win.result("8-row").view(torch.int16), a.cpu().view(torch.int16))


# ----------------------------------------------------------------------------- 6: end to end
def _e2e(dev, monkeypatch, tc, prompts, P, T, fp8_names):
    """`prompts` distinct prompts x 8 copies, greedy, teacher-forced on the bf16 rollout's tokens; the token loop streams e4m3 images of the
    projections `fp8_names` (asserted) and of the lm_head, bf16 packed images of the others.  Oracle: the installed HF Qwen3 in fp32 / bf16
    whose decode-step linears hold the DECODED images (the others their bf16 weights) -> (model, inputs, traced fp8 logits, rel to bf16 oracle)"""
    from bioreason_amd import configs, generation
    from bioreason_amd.modeling import Qwen3ForCausalLM
    from oracle import dna_llm_oracle as O
    monkeypatch.setenv("BRA_FP8_PREFILL", "0")        # the TOKEN LOOP against an oracle whose prompt K / V are bf16
    copies = 8
    B = prompts * copies
    H, F_, V = tc["hidden_size"], tc["intermediate_size"], tc["vocab_size"]
    Nq, Nkv = tc["num_attention_heads"] * tc["head_dim"], tc["num_key_value_heads"] * tc["head_dim"]
    m = Qwen3ForCausalLM(configs.qwen3_config(**tc), device=dev)
    m.init_weights(0.02, seed=1)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for n_, p_ in m.named_parameters():
            if "norm" in n_ and n_.endswith("weight"):
                p_.copy_((1.0 + 0.1 * torch.randn(p_.shape, generator=g)).to(p_.dtype).to(dev))
    eng = m.ensure_packed()
    emb = (torch.randn(prompts, P, H, generator=g) * 0.02).to(BF).to(dev).repeat_interleave(copies, 0)
    mask = torch.ones(B, P, dtype=torch.long, device=dev)
    mask[:, :5] = 0
    alias = [(b // copies) * copies for b in range(B)]
    kw = dict(max_new_tokens=T, do_sample=False, eos_token_id=None, prompt_alias=alias, use_graph=False)
    tok_bf = generation.generate(m, emb, mask, **kw)
    m.rollout_fp8 = True
    assert getattr(eng, "_head_fp8", None) is None
    tr8 = []
    tok_f8 = generation.generate(m, emb, mask, force_tokens=tok_bf, trace_logits=tr8, **kw)
    rw = generation.rollout_weights(m, rows=B)
    for R in rw:
        assert tuple(R.get("fp8_proj", ())) == tuple(fp8_names), (R.get("fp8_proj"), "the fp8 images were not built for these shapes")
        assert bool(R.get("fp8")) == (len(fp8_names) == 4)
    assert getattr(eng, "_head_fp8", None) is not None, "the step did not ask for the fp8 lm_head"       # (built on first use, by the step state)
    head_q, head_s = generation.packed_head_fp8(m, rows=B)
    assert len(tr8) == T - 1
    sd = {k: v.detach().float().cpu() for k, v in m.state_dict().items()}
    ora_bf = O.make_qwen3(tc, "eager")
    missing, _ = ora_bf.load_state_dict(sd, strict=False)
    assert not [k for k in missing if "lm_head" not in k], missing[:3]
    ora_bf.tie_weights()
    ora_bf.eval()
    ora_fq = copy.deepcopy(ora_bf)
    ora_fq.config.tie_word_embeddings = False
    wide = B > 8

    def dq(R, nm, N, K):        # (8 rows: diagonal tiles wherever the 8-row class uses them; 16 rows: 16-column tiles everywhere)
        diag = (not wide) and nm != "Wgu" and _diag8(N, K, False, False)
        return unpack_fp8_fast(R[nm + "_q"], N, K, diag).view(F8).float() * R[nm + "_s"].float().cpu()[:, None]
    for li, R in enumerate(rw):
        lay = ora_fq.model.layers[li]
        if "Wqkv" in fp8_names:
            wqkv = dq(R, "Wqkv", Nq + 2 * Nkv, H)
            lay.self_attn.q_proj.weight.data, lay.self_attn.k_proj.weight.data, lay.self_attn.v_proj.weight.data = \
                wqkv[:Nq].clone(), wqkv[Nq:Nq + Nkv].clone(), wqkv[Nq + Nkv:].clone()
            lay.input_layernorm.weight.data.fill_(1.0)                            # (folded into the quantised weights)
        if "Wo" in fp8_names:
            lay.self_attn.o_proj.weight.data = dq(R, "Wo", H, Nq)
        if "Wgu" in fp8_names:
            wgu = dq(R, "Wgu", 2 * F_, H).view(F_ // 8, 2, 8, H)                  # gate / up rows interleaved in blocks of 8
            lay.mlp.gate_proj.weight.data, lay.mlp.up_proj.weight.data = wgu[:, 0].reshape(F_, H).clone(), wgu[:, 1].reshape(F_, H).clone()
            lay.post_attention_layernorm.weight.data.fill_(1.0)
        if "Wd" in fp8_names:
            lay.mlp.down_proj.weight.data = dq(R, "Wd", H, F_)
    ora_fq.model.norm.weight.data.fill_(1.0)
    ora_fq.lm_head.weight = torch.nn.Parameter(unpack_fp8_fast(head_q, V, H, False).view(F8).float() * head_s.float().cpu()[:, None])
    assert ora_fq.lm_head.weight.data_ptr() != ora_fq.model.embed_tokens.weight.data_ptr()
    lead = [p * copies for p in range(prompts)]

    def oracle_steps(dtype):
        a, b = copy.deepcopy(ora_bf).to(dtype), copy.deepcopy(ora_fq).to(dtype)
        for mod in list(a.modules()) + list(b.modules()):                          # rotary buffers stay fp32, as from_pretrained leaves them
            if isinstance(getattr(mod, "inv_freq", None), torch.Tensor):
                mod.inv_freq = mod.inv_freq.float()
        per_prompt = []
        for r0 in lead:
            e1, am = emb[r0:r0 + 1].float().cpu().to(dtype), mask[r0:r0 + 1].cpu()
            logits = []
            with torch.no_grad():
                past = a.model(inputs_embeds=e1, attention_mask=am, use_cache=True).past_key_values
                for t in range(T - 1):
                    tok = tok_bf[r0, t].cpu().view(1, 1)
                    am = torch.cat([am, torch.ones(1, 1, dtype=am.dtype)], 1)
                    out = b(inputs_embeds=a.model.embed_tokens(tok), attention_mask=am, past_key_values=past, use_cache=True)
                    past = out.past_key_values
                    logits.append(out.logits[0, -1].float())
            per_prompt.append(torch.stack(logits))
        return torch.stack(per_prompt)                                             # [prompts, T - 1, V]
    ref32, ref16 = oracle_steps(torch.float32), oracle_steps(torch.bfloat16)
    got = torch.stack([torch.stack([t_[r0].float().cpu() for t_ in tr8]) for r0 in lead])
    e_hip, e_ref = rel(got, ref32), rel(ref16, ref32)
    print(f"\n[fp8-rows16] {B} rows, fp8 {fp8_names}: rel(hip, fp32) {e_hip:.3e}, rel(oracle bf16, fp32) {e_ref:.3e}")
    assert e_hip <= 1.25 * e_ref, f"fp8 rollout: rel(hip, fp32) {e_hip:.3e} > 1.25 x rel(oracle bf16, fp32) {e_ref:.3e}"
    n_tie = 0
    for p, r0 in enumerate(lead):
        for t in range(T - 1):
            ours, theirs = int(tok_f8[r0, t + 1]), int(ref32[p, t].argmax())
            if ours != theirs:
                margin = (ref32[p, t, theirs] - ref32[p, t, ours]).item()
                assert 0 <= margin <= 3.0 * e_ref * ref32[p, t].norm().item() / V ** 0.5 + 1e-3, (p, t, ours, theirs, margin)
                n_tie += 1
        for j in range(1, copies):
            assert torch.equal(tok_f8[r0 + j], tok_f8[r0])                          # copies of one prompt, teacher-forced: identical
    assert n_tie <= 2
    return m, emb, mask, tok_bf, kw, got


@pytest.mark.gpu
def test_rollout_at_16_rows_streams_fp8_images_against_the_oracle(hip_device, monkeypatch):
    """(a) Qwen3-1.7B widths, 2 layers, V = 8192, two prompts x 8 copies: every layer and the head stream e4m3 at rows = 16; with
    BRA_FP8_WIDE=0 the images are bf16 again and the logits move by quantisation noise — not by nothing, not by garbage"""
    from bioreason_amd import generation
    tc = dict(vocab_size=8192, hidden_size=2048, intermediate_size=6144, num_hidden_layers=2, num_attention_heads=16, num_key_value_heads=8,
              head_dim=128, rope_theta=1e6, max_position_embeddings=4096)
    m, emb, mask, tok_bf, kw, got = _e2e(hip_device, monkeypatch, tc, 2, 200, 12, ("Wqkv", "Wo", "Wgu", "Wd"))
    monkeypatch.setenv("BRA_FP8_WIDE", "0")
    trb = []
    generation.generate(m, emb, mask, force_tokens=tok_bf, trace_logits=trb, **kw)
    assert not any(R.get("fp8_proj") or R.get("fp8") for R in generation.rollout_weights(m, rows=16))
    d = rel(got, torch.stack([torch.stack([t_[r0].float().cpu() for t_ in trb]) for r0 in (0, 8)]))
    assert 2e-3 < d < 0.15, d


MIXED = dict(vocab_size=2048, hidden_size=1024, intermediate_size=1280, num_hidden_layers=1, num_attention_heads=8, num_key_value_heads=2,
             head_dim=128, rope_theta=1e6, max_position_embeddings=4096)


def test_the_mixed_widths_refuse_exactly_the_down_projection(backend):
    """the library's own answers for the widths of the mixed-layer test, in both row classes"""
    H, F_, Nqkv, Nq = 1024, 1280, 1536, 1024
    for rows in (8, 16):
        for (N, K, act, want) in ((Nqkv, H, False, True), (H, Nq, False, True), (2 * F_, H, True, True), (H, F_, False, False)):
            got = ops.dec_pack_weights_fp8(rnd(N, K, dev=backend, scale=0.05), act=act, rows=rows)
            assert (got is not None) == want, (rows, N, K)
        assert ops.dec_pack_weights(rnd(H, F_, dev=backend, scale=0.05), rows=rows) is not None      # the bf16 image the step streams instead
        assert ops.dec_pack_weights_fp8(rnd(2048, H, dev=backend, scale=0.05), out_f32=True, rows=rows) is not None


@pytest.mark.gpu
@pytest.mark.parametrize("prompts", [1, 2])
def test_rollout_over_mixed_fp8_and_bf16_layers_against_the_oracle(hip_device, monkeypatch, prompts):
    """(b) widths whose down projection (K = 1280) no fp8 form takes, at 8 and at 16 rows: Wqkv, Wo and Wgu stream e4m3, Wd its bf16 packed
    image in the same step; the oracle keeps down_proj at its bf16 weight"""
    _e2e(hip_device, monkeypatch, MIXED, prompts, 200, 12, ("Wqkv", "Wo", "Wgu"))


def test_rollout_fp8_at_16_rows_falls_back_to_bf16_where_the_shapes_do_not_fit(backend):
    """(c) test_rollout_fp8_falls_back_to_bf16_where_the_shapes_do_not_fit at two prompts x 8 copies, on that test's fixture (tiny_b: hidden
    256, intermediate 512): no layer is an fp8 layer (`fp8` = all four projections), there is no W8A8 prompt pass and no fp8 lm_head, the
    greedy tokens are the bf16 rollout's, the flag never fails a run.  The down projection alone has an image in the 16-row class (K = 512,
    four waves x four chunks; the 8-row class has none) and streams it next to three bf16 images."""
    from test_decode_rows32 import _tiny_b, _inputs
    from bioreason_amd import generation
    fix, m, b = _tiny_b(backend)
    inp = _inputs(b, [0] * 8 + [1] * 8, [0] * 8 + [8] * 8)
    kw = dict(max_new_tokens=5, do_sample=False, eos_token_id=None, use_graph=False)
    want = m.generate(**inp, **kw)
    m.text_model.rollout_fp8 = True
    assert generation.rollout_fp8_enabled(m.text_model)
    got = m.generate(**inp, **kw)
    assert got.shape[0] == 16 and torch.equal(got, want)
    rw = generation.rollout_weights(m.text_model, rows=16)
    assert not any(R.get("fp8") or R.get("rm8") for R in rw)
    assert all(tuple(R.get("fp8_proj", ())) == ("Wd",) for R in rw)
    assert generation.packed_head_fp8(m.text_model, rows=16) is None                      # (hidden 256: no head image in either class)
    m.text_model.rollout_fp8 = False
    assert not any(R.get("fp8_proj") for R in generation.rollout_weights(m.text_model, rows=16))
