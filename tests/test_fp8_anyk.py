"""fp8 (OCP e4m3) rollout weights at any K % 64 == 0, 1 .. 32 rows, for the plain role of the decode step (o_proj, down_proj: no norm, bf16
output, optional residual and statistics): bra_dec_pack_weights_fp8_anyk, bra_dec_gemm2_fp8_anyk, bra_dec_gemm2_fp8_anyk_ok
(k_decgemm8.hip: dec_f8k_kernel), the step driver's choice between the single-round forms and this one (k_decode.hip) and
generation.rollout_weights under BRA_FP8_ANYK=1.  Helpers and allowances are those of tests/test_gemm_family_rowwise.py,
tests/test_decode_proj_rowwise.py, tests/test_fp8_rollout.py and tests/test_fp8_rows16.py.

  packer   at a K the rows = 16 packer takes, the same bytes; elsewhere the nearest-even statement of
           test_fp8_rollout.test_fp8_pack_is_nearest_even_quantisation over the image un-permuted with 16-column tiles.
  exact    W integers in [-7, 7] with a 7 in every row (scale 2^-6, codes 64 W, both asserted), x integers |v| <= 2: every partial sum is
           below 2 * 448 * 17408 < 2^24 (asserted), so outputs are rnd(acc) and rnd(rnd(acc) + res) bit for bit and ss_out is exact.
           K: one wave with a pair (64), empty waves (192), four full waves (960), eight waves x 4 requests in one round (1280) and in two
           (3008, 4096), eight waves x 5 requests in four rounds (9728: a last round of four) and seven (17408).
  rows     random values: rows of an M = 32 call against M = 16 calls on both halves and an M = 5 call, outputs and ss_out bit for bit.
  random   every element against float64 over the codes and scales read back, under test_decode_proj_rowwise's fp8 no-norm allowance.
  host     tiny_b under BRA_FP8_ANYK=1 at 8, 16 and 32 rows; GPU: the oracle criterion of test_fp8_rows16._e2e on the mixed widths (all four
           projections now e4m3) and at Qwen3-4B widths, where the W8A8 prompt pass then engages.

Emulator cases above EMU_MAX weight elements are skipped; each names the smaller case of the same form that runs there."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bioreason_amd import generation, ops, _lib                                                          # noqa: E402
from test_gemm_family_rowwise import _bf, _assert_bits, _ties, _ratio, _randint, _Window                 # noqa: E402
from test_decode_proj_rowwise import _check_ss, _bound_ref, _assert_ratios, EMU_MAX, UNSUPPORTED         # noqa: E402
from test_fp8_rollout import unpack_fp8_fast, rel, rnd                                                   # noqa: E402
import test_fp8_rows16                                                                                  # noqa: E402
from test_fp8_rows16 import _e2e, _emu_skip, MIXED                                                       # noqa: E402
from test_decode_rows32 import _tiny_b, _inputs as _tiny_inputs, _Counter, BATCHES                       # noqa: E402

BF, F32, F64, F8 = torch.bfloat16, torch.float32, torch.float64, torch.float8_e4m3fn
ARG = _lib.BRA_ERR_ARG
GRID_CAP = {4: 512, 8: 256}             # workgroups by waves (k_decgemm8.hip: df8_grid_cap)


def _waves(K):
    return 8 if K // 64 >= 16 else 4


def _call(x, q, sc, win, M, N, K, res=None, sw=None, ldx=None, ldres=None):
    some = next(t for t in (x, q, sc) if t is not None)
    return _lib.get_lib().call_rc("bra_dec_gemm2_fp8_anyk", x, x.stride(0) if ldx is None else ldx, q, sc, res,
                                  (res.stride(0) if res is not None else 0) if ldres is None else ldres, win.win if win is not None else None,
                                  win.win.stride(0) if win is not None else 0, sw.win if sw else None, sw.win.stride(0) if sw else 0, M, N, K,
                                  _lib.current_stream(some))


def _ok(N, K):
    return bool(_lib.get_lib()._dll.bra_dec_gemm2_fp8_anyk_ok(int(N), int(K)))


# ----------------------------------------------------------------------------- 1: the packer
@pytest.mark.parametrize("K", [512, 2048, 4096])
def test_packer_writes_the_rows16_image_where_both_exist(backend, K):
    N = 48
    W = rnd(N, K, dev=backend, scale=0.05, seed=K)
    W[1] = 0
    q, sc = ops.dec_pack_weights_fp8_anyk(W)
    q16, s16 = ops.dec_pack_weights_fp8(W, rows=16)
    assert q.dtype == torch.uint8 and tuple(q.shape) == (N, K) and tuple(sc.shape) == (N,)
    assert torch.equal(q.cpu(), q16.cpu()) and torch.equal(sc.cpu().view(torch.int32), s16.cpu().view(torch.int32))


@pytest.mark.parametrize("K", [64, 1280, 9728])
def test_packer_is_nearest_even_quantisation_at_any_k(backend, K):
    """the statement of test_fp8_rollout.test_fp8_pack_is_nearest_even_quantisation, at K the single-round packer refuses"""
    N = 48
    assert ops.dec_pack_weights_fp8(rnd(N, K, dev=backend), rows=16) is None and ops.dec_pack_weights_fp8(rnd(N, K, dev=backend)) is None
    W = rnd(N, K, dev=backend, scale=0.05, seed=1)
    W[3, 5] = 0.0
    W[1] = 0                                                                     # an all-zero row: scale 1, codes 0
    got = ops.dec_pack_weights_fp8_anyk(W)
    assert got is not None
    q, scale = got
    codes = unpack_fp8_fast(q, N, K, False)
    wf = W.float().cpu()
    amax = wf.abs().amax(1)
    want_scale = torch.where(amax > 0, amax * (1.0 / 448.0), torch.ones_like(amax))
    assert torch.allclose(scale.cpu(), want_scale, rtol=1e-6, atol=0)
    t = wf * (1.0 / scale.cpu())[:, None]                                        # the pack kernel multiplies by the reciprocal
    want = t.to(F8).view(torch.uint8)
    same = codes == want
    if not bool(same.all()):                                                     # (1 ulp of the reciprocal: either neighbour at a rounding boundary)
        dec_got, dec_want = codes.view(F8).float(), want.view(F8).float()
        bad = ~same
        mid = 0.5 * (dec_got[bad] + dec_want[bad])
        assert ((t[bad] - mid).abs() <= 2e-6 * t[bad].abs() + 1e-12).all(), "a code is not the nearest e4m3 value"
        assert bad.sum() <= max(4, N * K // 20000)
    assert (codes[1] == 0).all() and scale[1].item() == 1.0
    assert int(codes.view(F8).float().abs().max()) == 448


def test_packer_refuses_partial_tiles_and_odd_step_counts(backend):
    lib = _lib.get_lib()
    for N, K in ((40, 128), (48, 96)):
        assert not _ok(N, K)
        W = rnd(N, K, dev=backend)
        q, sc = torch.full((N, K), 7, dtype=torch.uint8, device=backend), torch.full((N,), 3.0, device=backend)
        assert lib.call_rc("bra_dec_pack_weights_fp8_anyk", W, K, N, K, q, sc, _lib.current_stream(W)) == UNSUPPORTED
        assert bool((q == 7).all()) and bool((sc == 3.0).all())
        assert ops.dec_pack_weights_fp8_anyk(W) is None
    W = rnd(48, 128, dev=backend)
    q, sc = torch.zeros(48, 128, dtype=torch.uint8, device=backend), torch.zeros(48, device=backend)
    for args in ((None, 128, 48, 128, q, sc), (W, 128, 48, 128, None, sc), (W, 128, 48, 128, q, None), (W, 132, 48, 128, q, sc)):
        with pytest.raises(_lib.KernelError) as e:
            lib.call("bra_dec_pack_weights_fp8_anyk", *args, _lib.current_stream(W))
        assert e.value.status == ARG
    assert int(q.sum()) == 0 and float(sc.sum()) == 0.0


# ----------------------------------------------------------------------------- 2: the exact set
@functools.lru_cache(maxsize=16)
def _exact_inputs(N, K):
    g = torch.Generator().manual_seed(31 * N + K)
    x, W, res = _randint(g, (32, K), 2), _randint(g, (N, K), 7), _randint(g, (32, N), 256)
    W[torch.arange(N), torch.randint(0, K, (N,), generator=g)] = 7.0
    assert (x.abs() @ (64 * W).abs().T).max() < 2 ** 24
    return {"x": x.to(BF), "W": W.to(BF), "res": res.to(BF)}


def _pack_exact(dev, d, N, K):
    got = ops.dec_pack_weights_fp8_anyk(d["W"].to(dev))
    assert got is not None
    q, sc = got
    assert (sc.cpu() == 2.0 ** -6).all()
    assert torch.equal(unpack_fp8_fast(q, N, K, False).view(F8).to(F64), 64 * d["W"].to(F64))
    return q, sc


def _exact_case(dev, M, N, K, with_res, tally):
    name = f"fp8-anyk-{'res' if with_res else 'bf16'}-{M}x{N}x{K}"
    d = _exact_inputs(N, K)
    q, sc = _pack_exact(dev, d, N, K)
    x = d["x"][:M].contiguous().to(dev)
    ntiles = N // 16
    win = _Window(M, N, BF, dev, "direct" if M % 2 else "lds")
    res = d["res"][:M].contiguous().to(dev) if with_res else None
    sw = _Window(M, ntiles, F32, dev, "direct") if with_res else None
    assert _call(x, q, sc, win, M, N, K, res=res, sw=sw) == 0, name
    got = win.result(name)                                                       # (rows >= M and everything around the window: untouched)
    acc, R = d["x"][:M].to(F64) @ d["W"].to(F64).T, d["res"][:M].to(F64)
    want = (_bf(acc) + R).to(BF) if with_res else acc.to(BF)
    tally["ties"] = tally.get("ties", 0) + _ties(acc) + (_ties(_bf(acc) + R) if with_res else 0)
    _assert_bits(name, got, want)
    if with_res:
        tally["ss_exact"] = tally.get("ss_exact", 0) + _check_ss(name, sw.result(name + " ss_out"), got, 16, ntiles)


@pytest.mark.parametrize("M", [1, 8, 13, 16, 17, 32])
@pytest.mark.parametrize("K", [64, 192, 960, 1280, 3008, 4096, 9728, 17408])
def test_exact_every_k_every_row_count(backend, K, M):
    tally = {}
    for with_res in (False, True):
        _exact_case(backend, M, 48, K, with_res, tally)
    assert tally["ss_exact"] > 0
    assert K < 960 or M == 1 or tally["ties"] > 0, tally


# ----------------------------------------------------------------------------- 3: later tiles of a workgroup
@pytest.mark.parametrize("M,N,K,smaller", [(5, 8208, 192, None), (24, 8208, 192, None), (24, 4112, 3008, "24 x 8208 x 192 (tiles) and 17 x 48 x 3008 (rounds)")])
def test_exact_later_tiles_of_a_workgroup(backend, M, N, K, smaller):
    """more tiles than the grid cap: the weight stream runs on across the tile seam, the epilogue wave rotates, the slabs alternate, the
    residual of a later tile is loaded in the epilogue; at K = 3008 a tile is two rounds, so the seam falls between items of one stream"""
    if smaller:
        _emu_skip(backend, N, K, smaller)
    assert N // 16 > GRID_CAP[_waves(K)]
    tally = {}
    _exact_case(backend, M, N, K, True, tally)
    assert tally["ties"] > 0 and tally["ss_exact"] > 0


# ----------------------------------------------------------------------------- 4: a row does not depend on M
def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)


@pytest.mark.parametrize("K", [1280, 9728])
def test_rows_do_not_depend_on_the_row_count(backend, K):
    N = 48
    x, W, r = rnd(32, K, dev=backend, seed=3), rnd(N, K, dev=backend, scale=0.05, seed=4), rnd(32, N, dev=backend, seed=6)
    q, sc = ops.dec_pack_weights_fp8_anyk(W)

    def run(lo, hi):
        y, ss = ops.dec_gemm2_fp8_anyk(x[lo:hi].contiguous(), q, sc, res=r[lo:hi].contiguous(), want_ss=True)
        return _bits(y), _bits(ss[:hi - lo, :N // 16]), ss
    y32, s32, raw = run(0, 32)
    assert tuple(raw.shape)[0] == 32 and float(raw[:, N // 16:].abs().sum()) == 0.0          # the columns past N / 16 stay zero
    assert int((y32 != 0).sum()) > 0
    for lo, hi in ((0, 16), (16, 32), (0, 5)):
        y, s, _ = run(lo, hi)
        assert torch.equal(y, y32[lo:hi]) and torch.equal(s, s32[lo:hi]), (lo, hi)


# ----------------------------------------------------------------------------- 5: random values, element by element
@pytest.mark.parametrize("M", [8, 16, 32])
@pytest.mark.parametrize("K", [1280, 9728])
def test_random_rowwise(backend, K, M):
    """each element against float64 over the codes and scales read back: test_decode_proj_rowwise's bound and margin of the fp8 no-norm
    residual form (_bound_ref with c_epi = 3, MARGIN['f8_res'])"""
    N = 48
    g = torch.Generator().manual_seed(977 * M + K)
    x, W = (torch.randn(M, K, generator=g, dtype=F64) * 0.5).to(BF), (torch.randn(N, K, generator=g, dtype=F64) * 0.5).to(BF)
    R = torch.randn(M, N, generator=g, dtype=F64).to(BF)
    q, sc = ops.dec_pack_weights_fp8_anyk(W.to(backend))
    Wq = unpack_fp8_fast(q, N, K, False).view(F8).to(F64) * sc.cpu().to(F64)[:, None]
    win = _Window(M, N, BF, backend, "direct" if M % 2 else "lds")
    sw = _Window(M, N // 16, F32, backend, "direct")
    name = f"fp8-anyk-rand-{M}x{N}x{K}"
    assert _call(x.to(backend), q, sc, win, M, N, K, res=R.to(backend), sw=sw) == 0
    got = win.result(name)
    ref, E = _bound_ref(x.to(F64), Wq, K, "res", R.to(F64), c_epi=3)
    ratios = {"f8_res": _ratio((got.to(F64) - ref).abs(), E)}
    _check_ss(name, sw.result(name + " ss_out"), got, 16, N // 16)
    _assert_ratios(name, ratios, backend)


# ----------------------------------------------------------------------------- 6: refusals
def test_refusals_leave_every_buffer_untouched(backend):
    N, K = 48, 192
    x33 = rnd(33, K, dev=backend)
    W = rnd(N, K, dev=backend, scale=0.05)
    q, sc = ops.dec_pack_weights_fp8_anyk(W)
    r33 = rnd(33, N, dev=backend)

    def refused(want, M, N_, K_, x=x33, q_=q, sc_=sc, out=True, **kw):
        win, sw = _Window(max(M, 1), N_, BF, backend), _Window(max(M, 1), 32, F32, backend, "direct")
        args = (x, q_, sc_, win if out else None, M, N_, K_)
        if want == ARG:
            with pytest.raises(_lib.KernelError) as e:
                _call(*args, res=r33, sw=sw, **kw)
            assert e.value.status == ARG
        else:
            assert _call(*args, res=r33, sw=sw, **kw) == UNSUPPORTED
        win.result("refused")
        sw.result("refused ss_out")
        assert torch.equal(win.buf.cpu(), win.before) and torch.equal(sw.buf.cpu(), sw.before)
    refused(ARG, 0, N, K)
    refused(UNSUPPORTED, 33, N, K)
    refused(ARG, 8, N, K, x=None, ldx=K)
    refused(ARG, 8, N, K, q_=None)
    refused(ARG, 8, N, K, sc_=None)
    refused(ARG, 8, N, K, out=False)
    refused(ARG, 8, N, K, ldx=K + 4)                                             # ldx % 8 != 0
    refused(ARG, 8, N, K, ldres=N + 2)                                           # ldres % 4 != 0
    refused(UNSUPPORTED, 8, N, 96)                                               # K % 64 != 0
    refused(UNSUPPORTED, 8, 40, K)                                               # N % 16 != 0
    # the exported rule agrees with what the call does
    for N_, K_ in ((48, 64), (48, 192), (16, 17408), (48, 96), (40, 192), (48, 32), (0, 64), (48, 0), (-16, 64)):
        ok = _ok(N_, K_)
        assert ok == (N_ > 0 and K_ > 0 and N_ % 16 == 0 and K_ % 64 == 0), (N_, K_)
        assert ops.dec_gemm2_fp8_anyk_ok(N_, K_) == ok
        if N_ > 0 and K_ >= 32:
            xx = rnd(4, K_, dev=backend)
            qq, ss = torch.zeros(N_, K_, dtype=torch.uint8, device=backend), torch.ones(N_, device=backend)
            win = _Window(4, N_, BF, backend)
            assert _call(xx, qq, ss, win, 4, N_, K_) == (0 if ok else UNSUPPORTED), (N_, K_)
            win.result("rule")
            assert ok or torch.equal(win.buf.cpu(), win.before)


# ----------------------------------------------------------------------------- 7: the host, on the tiny fixture
def _expected_fp8_proj(tm, rows, dev):
    """the library's own rules: a projection is e4m3 where the single-round packer of the row class takes it, and a plain one (o, down) also
    where bra_dec_gemm2_fp8_anyk_ok says so"""
    eng = tm.ensure_packed()
    prows = 16 if rows > 8 else 8
    shapes = (("Wqkv", eng.Nq + 2 * eng.Nkv, eng.H, True), ("Wo", eng.H, eng.Nq, False), ("Wgu", 2 * eng.F, eng.H, True), ("Wd", eng.H, eng.F, False))
    names = []
    for nm, N, K, normed in shapes:
        nw = torch.ones(K, dtype=BF, device=dev) if normed else None
        single = ops.dec_pack_weights_fp8(rnd(N, K, dev=dev, scale=0.05), act=(nm == "Wgu"), norm_w=nw, rows=prows) is not None
        if rows > 16:
            single = single and generation.fp8_rows32_form_exists(K, normed)
        if single or (not normed and _ok(N, K)):
            names.append(nm)
    return tuple(names)


def test_host_builds_and_streams_the_any_k_images_on_the_tiny_fixture(backend, monkeypatch):
    """tiny_b (hidden 256, q width 256, intermediate 512) under rollout_fp8 + BRA_FP8_ANYK=1: o and down stream e4m3 in every row class (the
    single-round forms take the down projection at 16 and 32 rows only), one prefill per loop; the 32-row loop's teacher-forced logits
    equal the 16-row loops' bit for bit on the 4 x 8 batch; with the switch unset the weight set is what it was"""
    fix, m, b = _tiny_b(backend)
    cfg = fix["config"]
    tm = m.text_model
    T = cfg["gen_tokens"]
    rows, alias = BATCHES["4x8"]
    want = fix["fp32_lora"]["greedy_ids"][rows].to(backend)
    tm.rollout_fp8 = True
    # the parent's weight sets, switch unset
    assert "BRA_FP8_ANYK" not in os.environ and generation._SWITCHES["BRA_FP8_ANYK"] == "0"
    assert all(tuple(R.get("fp8_proj", ())) == () for R in generation.rollout_weights(tm, rows=8))
    assert all(tuple(R.get("fp8_proj", ())) == ("Wd",) for R in generation.rollout_weights(tm, rows=16))
    monkeypatch.setenv("BRA_FP8_ANYK", "1")
    monkeypatch.setenv("BRA_DEC_ROWS32", "1")
    cnt = _Counter(monkeypatch)
    forced = dict(max_new_tokens=T, do_sample=False, eos_token_id=None, use_graph=False)
    traces = {}
    for B in (8, 16, 32):
        inp = _tiny_inputs(b, rows[:B], alias[:B])
        cnt.reset()
        traces[B] = []
        out = m.generate(**inp, trace_logits=traces[B], force_tokens=want[:B], **forced)
        assert (cnt.prefills, cnt.chunked) == (1, 0) and tuple(out.shape) == (B, T)
        rw = generation.rollout_weights(tm, rows=B)
        names = _expected_fp8_proj(tm, B, backend)
        assert names == ("Wo", "Wd")
        assert all(tuple(R.get("fp8_proj", ())) == names for R in rw), (B, rw[0].get("fp8_proj"))
        assert not any(R.get("fp8") or R.get("rm8") for R in rw)
        assert bool(torch.isfinite(traces[B][-1]).all()) and float(traces[B][-1].abs().max()) > 0
    assert generation.rollout_weights(tm, rows=32) is generation.rollout_weights(tm, rows=16)          # one image set
    # 32 rows in one loop against the 16-row chunks (BRA_FP8_ROWS32=0), the comparison of test_fp8_rows32 on this batch
    monkeypatch.setenv("BRA_FP8_ROWS32", "0")
    cnt.reset()
    tr16 = []
    inp = _tiny_inputs(b, rows, alias)
    f16 = m.generate(**inp, trace_logits=tr16, force_tokens=want, **forced)
    assert cnt.chunked == 1 and cnt.prefills >= 2
    assert len(traces[32]) == len(tr16) == T - 1
    for t, (a, c) in enumerate(zip(traces[32], tr16)):
        assert torch.equal(a.cpu(), c.cpu()), (t, (a.cpu() != c.cpu()).nonzero()[:4].tolist())
    # rows 0 .. 15 of the 16-row loop are the first chunk
    for t, (a, c) in enumerate(zip(traces[16], tr16)):
        assert torch.equal(a.cpu(), c[:16].cpu()), t
    monkeypatch.delenv("BRA_FP8_ROWS32")
    monkeypatch.delenv("BRA_FP8_ANYK")
    assert all(tuple(R.get("fp8_proj", ())) == ("Wd",) for R in generation.rollout_weights(tm, rows=16))
    assert all(tuple(R.get("fp8_proj", ())) == () for R in generation.rollout_weights(tm, rows=8))
    tm.rollout_fp8 = False
    assert not any(R.get("fp8_proj") for R in generation.rollout_weights(tm, rows=16))


# ----------------------------------------------------------------------------- 8: end to end on the GPU
ALL4 = ("Wqkv", "Wo", "Wgu", "Wd")


@pytest.mark.gpu
@pytest.mark.parametrize("prompts", [1, 2])
def test_rollout_on_the_mixed_widths_streams_all_four_projections_as_e4m3(hip_device, monkeypatch, prompts):
    """test_fp8_rows16's mixed widths (down projection: K = 1280) with BRA_FP8_ANYK=1, at 8 and at 16 rows: the down projection streams its
    any-K image, every layer is an fp8 layer; the oracle holds the decoded images.  At 8 rows the oracle's un-permutation is told that the
    any-K image is in 16-column order (the 8-row class's own images of N = hidden projections are in diagonal order)."""
    monkeypatch.setenv("BRA_FP8_ANYK", "1")
    diag8 = test_fp8_rows16._diag8

    def diag8_anyk(N, K, act, f32):
        single = ops.dec_pack_weights_fp8(rnd(N, K, dev=hip_device, scale=0.05), act=bool(act), out_f32=bool(f32), rows=8) is not None
        return diag8(N, K, act, f32) and single
    monkeypatch.setattr(test_fp8_rows16, "_diag8", diag8_anyk)
    m = _e2e(hip_device, monkeypatch, MIXED, prompts, 200, 12, ALL4)[0]
    assert generation.rollout_weights(m, rows=8 * prompts)[0].get("fp8") is True


QWEN3_4B = dict(vocab_size=8192, hidden_size=2560, intermediate_size=9728, num_hidden_layers=2, num_attention_heads=32, num_key_value_heads=8,
                head_dim=128, rope_theta=1e6, max_position_embeddings=4096)


@pytest.mark.gpu
def test_rollout_at_qwen3_4b_widths_streams_all_four_projections_and_runs_the_w8a8_prompt_pass(hip_device, monkeypatch):
    """Qwen3-4B widths x 2 layers, two prompts x 8 copies: o (K = 4096) streams its single-round image, down (K = 9728) its any-K image, so
    every layer is an fp8 layer — `fp8`, `rm8`, the e4m3 lm_head — against the oracle under _e2e's criterion; then the W8A8 prompt pass
    (BRA_FP8_PREFILL=1) engages and moves the logits by the interval
    test_fp8_rollout.test_fp8_prompt_pass_and_reference_pass_in_a_step_at_qwen3_widths asserts for the same comparison"""
    monkeypatch.setenv("BRA_FP8_ANYK", "1")
    m, emb, mask, tok_bf, kw, got = _e2e(hip_device, monkeypatch, QWEN3_4B, 2, 200, 12, ALL4)
    assert generation.prefill_fp8_weights(m, 16) is None                          # (_e2e: bf16 prompt pass)
    monkeypatch.setenv("BRA_FP8_PREFILL", "1")
    m.ensure_packed()._rollout = None                                             # (the cached set has no row-major images)
    assert generation.prefill_fp8_weights(m, 16) is not None
    rw = generation.rollout_weights(m, rows=16)
    assert all(tuple(R["fp8_proj"]) == ALL4 and R.get("fp8") and R.get("rm8") is not None for R in rw)
    tr = []
    generation.generate(m, emb, mask, force_tokens=tok_bf, trace_logits=tr, **kw)
    w8 = torch.stack([torch.stack([t_[r0].float().cpu() for t_ in tr]) for r0 in (0, 8)])
    d = rel(w8, got)
    print(f"\n[fp8-anyk] Qwen3-4B widths: W8A8 prompt pass against the bf16 prompt pass, rel {d:.3e}")
    assert 1e-3 < d < 0.25, d
