"""fp8 (OCP e4m3) rollout weights at 17 .. 32 rows: bra_dec_gemm2_fp8_rows(image_rows = 32) (k_decgemm.hip: dec_gemm2_kernel<.., WIDE = 2, ..,
F8 = 1>), bra_dec_gemm2_fp8_rows32_ok, the step driver's row class (k_decode.hip) and the host's one token loop over e4m3 images
(generation.rollout_weights, _one_loop_ok, BRA_FP8_ROWS32).  The form streams the rows = 16 image — there is no second image — and every
16-byte request feeds both 16-row halves of the batch.

The claim is exact: row r of a 32-row fp8 launch is BIT-IDENTICAL to row r of a 16-row fp8 launch (image_rows = 16) on the same image and
inputs.  As in tests/test_decode_rows32.py a row block shorter than 9 rows (M = 17 .. 24: rows [16, M)) is extended to 9 rows with the
buffer rows that follow it, because 8 rows or fewer select the 8-row kernels, which reduce K in another order over another image.

Bit-equality alone is self-consistency, so the form is also held to float64 on the integer-valued set of tests/test_fp8_rows16.py (scale
2^-6 and codes 64 W asserted, every partial sum below 2^24: outputs equal the float64 product bit for bit), SwiGLU by
test_decode_proj_rowwise's rule, and the folded statistics row by row with the one-hot probe: rows 16 .. 31 take their own rstd.

Helpers, value sets and allowances are those of tests/test_fp8_rows16.py, tests/test_decode_proj_rowwise.py and tests/test_decode_rows32.py.
Emulator cases above 4.3e6 weight elements are skipped; each names the smaller case of the same form that runs there."""
import os
import re
import shutil
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bioreason_amd import generation, ops, _lib                                              # noqa: E402
from test_gemm_family_rowwise import _bf, _assert_bits, _ties, _Window, U32                  # noqa: E402
from test_decode_proj_rowwise import (_fp8_inputs, _check_ss, _mirror, _pow2, _swiglu_twin, _assert_swiglu, _tau_rstd, _probe_stats,   # noqa: E402
                                      EPS, UNSUPPORTED, ROWS32_K)
from test_layer_glue_rowwise import NEAR_CAP                                                 # noqa: E402
from test_fp8_rollout import unpack_fp8_fast, rnd                                            # noqa: E402
from test_fp8_rows16 import FORMS, _call, _pack_exact, _act_inputs, _emu_skip                # noqa: E402
from test_decode_rows32 import _stats as _stats32, _tiny_b, _inputs as _tiny_inputs, _Counter, BATCHES      # noqa: E402

BF, F32, F64, F8 = torch.bfloat16, torch.float32, torch.float64, torch.float8_e4m3fn
ROWS = (17, 24, 31, 32)


def _ok32(K, normed):
    return bool(_lib.get_lib()._dll.bra_dec_gemm2_fp8_rows32_ok(int(K), int(normed)))


def _same_bits(a, b):
    it = torch.int32 if a.dtype == F32 else torch.int16
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


# ----------------------------------------------------------------------------- 1: rows equal the 16-row fp8 kernel
ROLES = [("o/down", dict(N=48, res=True, stat=True)), ("qkv", dict(N=48, norm=True)), ("gate/up", dict(N=96, norm=True, act=True)),
         ("lm_head", dict(N=48, norm=True, f32=True, stat=True))]


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("K", list(FORMS))
def test_rows_equal_the_16_row_fp8_kernel(backend, K, M):
    """every role at every single-round K: rows 0 .. 15 against an image_rows = 16, M = 16 call, rows 16 .. M - 1 against a 16-row call on
    rows [16, 16 + max(M - 16, 9)); rows >= M of every output and statistics buffer keep their pattern (the windows check everything
    around [M, N]); the folded-norm roles at K = 6144 return BRA_ERR_UNSUPPORTED and leave every buffer as it was"""
    dev = backend
    mb = max(M - 16, 9)
    x = rnd(32, K, dev=dev, seed=1)
    nw = (1.0 + 0.1 * torch.randn(K, generator=torch.Generator().manual_seed(3))).to(BF).to(dev)
    ss = _stats32(x, dev)
    for name, r in ROLES:
        N, act, f32, norm = r["N"], bool(r.get("act")), bool(r.get("f32")), bool(r.get("norm"))
        W = rnd(N, K, dev=dev, scale=0.05, seed=2)
        res = rnd(32, N, dev=dev, seed=4) if r.get("res") else None
        got = ops.dec_pack_weights_fp8(W, act=act, out_f32=f32, norm_w=nw if norm else None, rows=16)
        assert got is not None, (name, K)
        q, sc = got
        No, nt = (N // 2 if act else N), N // 16

        def run(lo, m, image_rows):
            win = _Window(m, No, F32 if f32 else BF, dev, "direct" if m % 2 else "lds")
            sw = _Window(m, nt, F32, dev, "direct") if r.get("stat") else None
            rc = _call(x[lo:], q, sc, win, m, N, K, ss_in=ss[lo:] if norm else None, nss=ss.shape[1] if norm else 0,
                       res=res[lo:] if res is not None else None, sw=sw, act=act, f32=f32, image_rows=image_rows)
            return rc, win, sw
        rc, win, sw = run(0, M, 32)
        tag = f"{name} {M}x{N}x{K}"
        if norm and K == 6144:
            assert not _ok32(K, True)
            assert rc == UNSUPPORTED, (tag, rc)
            win.result(tag)
            assert torch.equal(win.buf.cpu(), win.before) and (sw is None or torch.equal(sw.buf.cpu(), sw.before)), tag
            continue
        assert rc == 0 and _ok32(K, norm), (tag, rc)
        y, s = win.result(tag), (sw.result(tag + " stat") if sw else None)
        rca, wa, swa = run(0, 16, 16)
        rcb, wb, swb = run(16, mb, 16)
        assert rca == 0 and rcb == 0, tag
        ya, yb = wa.result(tag + " a"), wb.result(tag + " b")
        assert _same_bits(y[:16], ya), tag                                         # rows 0 .. 15
        assert _same_bits(y[16:M], yb[:M - 16]), tag                               # rows 16 .. M - 1
        assert y.float().abs().max() > 0
        if s is not None:
            sa, sb = swa.result(tag + " stat a"), swb.result(tag + " stat b")
            assert _same_bits(s[:16], sa) and _same_bits(s[16:M], sb[:M - 16]), tag


# ----------------------------------------------------------------------------- 2: exact against float64
def _exact32(dev, M, N, K, epi, tally):
    """test_fp8_rows16._exact_case at 17 .. 32 rows (image_rows = 32)"""
    f32 = epi in ("f32", "f32max")
    m = _mirror(M, N, K, epi, False, 1)
    assert (m["form"].rows, m["form"].kind, (m["form"].nw, m["form"].nl)) == (32, "fast", FORMS[K]) and not m["refused"]
    name = f"fp8-32r-{m['form'].nw}x{m['form'].nl}-{epi}-{M}x{N}x{K}"
    d = _fp8_inputs(M, N, K, "exact")
    q, sc = _pack_exact(dev, d, N, K, f32=f32)
    x = d["x"].to(dev)
    win = _Window(M, N, F32 if f32 else BF, dev, "direct" if M % 2 else "lds")
    res = d["res"].to(dev) if epi == "res" else None
    sw = _Window(M, m["ntiles"], F32, dev, "direct") if epi in ("res", "f32max") else None
    rc = _call(x, q, sc, win, M, N, K, res=res, sw=sw, f32=f32, image_rows=32)
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


def _act32(dev, M, K):
    """test_fp8_rows16._act_case at 17 .. 32 rows: the first input set whose twin ALONE stays within the cap"""
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
    name = f"fp8-32r-act-{M}x{N}x{K}"
    assert _call(d["x"].to(dev), q, sc, win, M, N, K, act=True, image_rows=32) == 0, name
    _assert_swiglu(name, win.result(name), twin)


@pytest.mark.parametrize("M", [17, 32])
@pytest.mark.parametrize("K", list(FORMS))
def test_exact_every_form_every_epilogue(backend, K, M):
    """rows = 16 image + image_rows = 32, no norm: fp32 (+ tile maxima), bf16, residual + ss_out bit for bit against the float64 product,
    SwiGLU by its rule; rows >= M of every output keep the pattern they held"""
    tally = {}
    for epi in ("f32max", "f32", "bf16", "res"):
        _exact32(backend, M, 48, K, epi, tally)
    _act32(backend, M, K)
    assert tally["ss_exact"] > 0
    assert K < 1024 or tally["ties"] > 0, tally


@pytest.mark.parametrize("K", [512, 4096])
@pytest.mark.parametrize("nss", [32, 256])
@pytest.mark.parametrize("M", [17, 32])
def test_folded_statistics_per_row(backend, M, nss, K):
    """test_fp8_rows16's probe at 17 and 32 rows: out[m, n] = rstd_m scale[n] code[n, k_m] with scale = 2^-6 and code = 64 W a power of
    two, so out / W is the device's rstd of row m, held to tau_rstd u against rsqrt(sum of ALL nss columns of row m / K + eps); rows >= M
    of ss_in hold 1e30 and must not reach any row.  The rows' statistics differ by a factor (1 + 0.61 i), so a second half that took the
    rstd of rows 0 .. 15 is far outside the allowance — asserted on the reference numbers themselves."""
    N = 48
    ss, rstd = _probe_stats(M, nss, K)
    assert ss.shape[0] == 32 and (M == 32 or bool((ss[M:] == 1.0e30).all()))
    tau = _tau_rstd(nss) * U32
    assert ((rstd[16:M] - rstd[:M - 16]).abs() / rstd[16:M] > 1000 * tau).all()
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
    assert _call(x.to(BF).to(dev), q, sc, win, M, N, K, ss_in=ss.to(dev), nss=nss, f32=True, image_rows=32) == 0
    out = win.result(f"fp8-32r-probe-{M}-{nss}-{K}").to(F64)
    r = out / W[:, km].T
    err = (r - rstd[:, None]).abs() / rstd[:, None]
    assert (err <= tau).all(), (M, nss, K, "rows", sorted(set(torch.nonzero(err > tau)[:, 0].tolist())), err.max().item() / U32)


# ----------------------------------------------------------------------------- 3: later tiles of a workgroup
@pytest.mark.parametrize("M,N,K,cap,hip_only", [(24, 8208, 512, 512, False), (24, 4112, 2048, 256, True)])
def test_exact_later_tiles_of_a_workgroup(backend, M, N, K, cap, hip_only):
    """more tiles than the grid cap: weights and scales ping-pong, the epilogue waves of both halves rotate, the residual of both halves is
    loaded in the epilogue"""
    if hip_only:
        _emu_skip(backend, N, K, "K = 512, N = 8208 (the 512-workgroup cap of four waves)")
    tally = {}
    for epi in ("res", "f32max"):
        m = _exact32(backend, M, N, K, epi, tally)
        assert m["later"] and m["grid"] == cap
    assert tally["ties"] > 0 and tally["ss_exact"] > 0


# ----------------------------------------------------------------------------- 4: pairings and the exported rule
def test_pairings_of_image_rows_and_M(backend):
    """every (image_rows, M) pairing outside {8: M <= 8, 16: 9 .. 16, 32: 17 .. 32} returns BRA_ERR_UNSUPPORTED and writes nothing; the
    packer keeps refusing rows > 16"""
    N, K = 64, 2048
    x = rnd(32, K, dev=backend)
    W = rnd(N, K, dev=backend, scale=0.05)
    q16, sc16 = ops.dec_pack_weights_fp8(W, rows=16)
    res = rnd(32, N, dev=backend, seed=5)
    allowed = {8: range(1, 9), 16: range(9, 17), 32: range(17, 33)}
    seen = 0
    for image_rows in (8, 16, 32, 0, 12, 24, 33, 64, -1):
        for M in (1, 8, 9, 16, 17, 24, 32):
            if M in allowed.get(image_rows, ()):
                continue
            win = _Window(M, N, BF, backend)
            sw = _Window(M, 32, F32, backend, "direct")
            rc = _call(x, q16, sc16, win, M, N, K, res=res, sw=sw, image_rows=image_rows)
            assert rc == UNSUPPORTED, (image_rows, M, rc)
            win.result(f"{image_rows}/{M}")
            assert torch.equal(win.buf.cpu(), win.before) and torch.equal(sw.buf.cpu(), sw.before), (image_rows, M)
            seen += 1
    assert seen == 9 * 7 - (2 + 2 + 3)
    assert ops.dec_gemm2_fp8(x[:17].contiguous(), q16, sc16, image_rows=16) is None
    assert ops.dec_gemm2_fp8(x[:16].contiguous(), q16, sc16, image_rows=32) is None
    y = ops.dec_gemm2_fp8(x[:17].contiguous(), q16, sc16, image_rows=32)
    assert y is not None and tuple(y[0].shape) == (17, N)
    lib = _lib.get_lib()
    q, sc = torch.zeros(N, K, dtype=torch.uint8, device=backend), torch.zeros(N, device=backend)
    for rows in (17, 32):
        with pytest.raises(_lib.KernelError) as e:
            lib.call("bra_dec_pack_weights_fp8_rows", W, K, N, K, 0, 0, None, rows, q, sc, _lib.current_stream(W))
        assert e.value.status == _lib.BRA_ERR_ARG
    assert int(q.sum()) == 0 and float(sc.sum()) == 0.0


def test_the_exported_rule_is_the_launchers(backend):
    """bra_dec_gemm2_fp8_rows32_ok at every K of test_decode_proj_rowwise.ROWS32_K, both norm states: 1 exactly at the single-round K of the
    16-row fp8 class minus the folded norm at 6144, and exactly there the call runs; elsewhere BRA_ERR_UNSUPPORTED, buffers untouched"""
    assert set(FORMS) <= set(ROWS32_K)
    N, M = 48, 17
    for K in ROWS32_K:
        x = rnd(M, K, dev=backend)
        ss = ops.row_sumsq(x, 32)
        for normed in (False, True):
            ok = _ok32(K, normed)
            assert ok == (K in FORMS and not (normed and K == 6144)), (K, normed)
            assert generation.fp8_rows32_form_exists(K, normed) == ok
            nw = torch.ones(K, dtype=BF, device=backend) if normed else None
            got = ops.dec_pack_weights_fp8(rnd(N, K, dev=backend, scale=0.05), norm_w=nw, rows=16)
            assert (got is not None) == (K in FORMS), K
            # (no image of this K: the launcher refuses before anything is read)
            q, sc = got if got is not None else (torch.zeros(N, K, dtype=torch.uint8, device=backend), torch.ones(N, device=backend))
            win = _Window(M, N, BF, backend)
            rc = _call(x, q, sc, win, M, N, K, ss_in=ss if normed else None, nss=32 if normed else 0, image_rows=32)
            assert rc == (0 if ok else UNSUPPORTED), (K, normed, rc)
            out = win.result(f"rule-{K}-{normed}")
            if not ok:
                assert torch.equal(win.buf.cpu(), win.before), (K, normed)
            else:
                assert out.float().abs().max() > 0
    for K in (0, -64, 32, 544, 5120, 8192, 12288):
        assert not _ok32(K, False) and not _ok32(K, True), K


# ----------------------------------------------------------------------------- 5: the host, on the tiny fixture
@pytest.mark.parametrize("batch", ["3x8", "4x8"])
def test_one_token_loop_over_fp8_images_decodes_what_the_row_chunks_decode(backend, monkeypatch, batch):
    """rollout_fp8 + BRA_DEC_ROWS32=1 on tiny_b (hidden 256, intermediate 512: the K = 512 down projection alone has an e4m3 image — a mixed
    layer at 32 rows): ONE prefill, no chunk path; teacher-forced logits bit-equal at every step to BRA_FP8_ROWS32=0 (16-row chunks, the
    behaviour before this form), free greedy tokens equal.  3 x 8: rows 16 .. 23 against the 16-row loop over rows 8 .. 23, for the reason
    test_decode_rows32.test_one_token_loop_decodes_what_the_row_chunks_decode gives."""
    fix, m, b = _tiny_b(backend)
    cfg = fix["config"]
    rows, alias = BATCHES[batch]
    inp = _tiny_inputs(b, rows, alias)
    B, T = len(rows), cfg["gen_tokens"]
    want = fix["fp32_lora"]["greedy_ids"][rows].to(backend)
    tm = m.text_model
    tm.rollout_fp8 = True
    assert generation.rollout_fp8_enabled(tm)
    cnt = _Counter(monkeypatch)
    forced = dict(max_new_tokens=T, do_sample=False, eos_token_id=None, use_graph=False, force_tokens=want)
    free = dict(max_new_tokens=T, do_sample=False, eos_token_id=None, use_graph=False)
    monkeypatch.setenv("BRA_DEC_ROWS32", "1")
    tr32 = []
    f32 = m.generate(**inp, trace_logits=tr32, **forced)
    assert (cnt.prefills, cnt.chunked) == (1, 0)                     # one prefill, one loop
    cnt.reset()
    g32 = m.generate(**inp, **free)
    assert (cnt.prefills, cnt.chunked) == (1, 0)
    rw = generation.rollout_weights(tm, rows=B)
    assert all(tuple(R.get("fp8_proj", ())) == ("Wd",) for R in rw) and not any(R.get("fp8") or R.get("rm8") for R in rw)
    assert rw is generation.rollout_weights(tm, rows=32) and rw is generation.rollout_weights(tm, rows=16)      # one image set
    assert generation.packed_head_fp8(tm, rows=B) is None                                  # (hidden 256: no head image in any class)
    monkeypatch.setenv("BRA_FP8_ROWS32", "0")
    cnt.reset()
    tr16 = []
    f16 = m.generate(**inp, trace_logits=tr16, **forced)
    assert cnt.chunked == 1 and cnt.prefills >= 2                    # the switch restores the 16-row chunks
    g16 = m.generate(**inp, **free)
    assert f32.shape == f16.shape == g32.shape == g16.shape == (B, T)
    assert len(tr32) == len(tr16) == T - 1 and tr32[0].shape == (B, cfg["text"]["vocab_size"])
    if batch == "3x8":
        inp_b = _tiny_inputs(b, rows[8:24], [0] * 8 + [8] * 8)
        trb = []
        fb = m.generate(**inp_b, trace_logits=trb, **dict(forced, force_tokens=want[8:24]))
        gb = m.generate(**inp_b, **free)
        tr16 = [torch.cat([c[:16], d[8:]], 0) for c, d in zip(tr16, trb)]
        f16, g16 = torch.cat([f16[:16], fb[8:]], 0), torch.cat([g16[:16], gb[8:]], 0)
    for t, (a, c) in enumerate(zip(tr32, tr16)):
        assert torch.equal(a.cpu(), c.cpu()), (t, (a.cpu() != c.cpu()).nonzero()[:4].tolist())
    assert torch.equal(f32, f16) and torch.equal(g32, g16)
    monkeypatch.delenv("BRA_FP8_ROWS32")
    tm.rollout_fp8 = False
    assert not any(R.get("fp8_proj") for R in generation.rollout_weights(tm, rows=B))


# ----------------------------------------------------------------------------- 6: end to end on the GPU
TC = dict(vocab_size=8192, hidden_size=2048, intermediate_size=6144, num_hidden_layers=2, num_attention_heads=16, num_key_value_heads=8,
          head_dim=128, rope_theta=1e6, max_position_embeddings=4096)


@pytest.fixture(scope="module")
def big_model():
    """Qwen3-1.7B widths, 2 layers, V = 8192, built once for the GPU tests of this module"""
    from bioreason_amd import configs
    from bioreason_amd.modeling import Qwen3ForCausalLM
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _lib.reset_library()
    dev = torch.device("cuda:0")
    m = Qwen3ForCausalLM(configs.qwen3_config(**TC), device=dev)
    m.init_weights(0.02, seed=1)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for n_, p_ in m.named_parameters():
            if "norm" in n_ and n_.endswith("weight"):
                p_.copy_((1.0 + 0.1 * torch.randn(p_.shape, generator=g)).to(p_.dtype).to(dev))
    m.ensure_packed()
    return m


def _prompts(m, prompts, P, dev):
    g = torch.Generator().manual_seed(5)
    emb = (torch.randn(prompts, P, TC["hidden_size"], generator=g) * 0.02).to(BF).to(dev).repeat_interleave(8, 0)
    mask = torch.ones(prompts * 8, P, dtype=torch.long, device=dev)
    mask[:, :5] = 0
    return emb, mask, [(r // 8) * 8 for r in range(prompts * 8)]


@pytest.mark.gpu
@pytest.mark.parametrize("prompts", [3, 4])
def test_rollout_at_24_and_32_rows_streams_fp8_images_in_one_loop(hip_device, monkeypatch, big_model, prompts):
    """every layer streams all four projections and the head as e4m3 in ONE token loop; teacher-forced logits bit-equal to the
    BRA_FP8_ROWS32=0 chunks — held to the fp32 oracle by tests/test_fp8_rows16.py — under the 3 x 8 rule of the tiny test; at 4 x 8 graph
    replay equals launch-by-launch over 40 tokens, and with the W8A8 prompt pass on the rollout completes inside the vocabulary"""
    m, dev = big_model, hip_device
    B, P, T, V = prompts * 8, 200, 12, TC["vocab_size"]
    emb, mask, alias = _prompts(m, prompts, P, dev)
    monkeypatch.setenv("BRA_FP8_PREFILL", "0")
    monkeypatch.setenv("BRA_DEC_ROWS32", "1")
    m.rollout_fp8 = True
    try:
        cnt = _Counter(monkeypatch)
        kw = dict(max_new_tokens=T, do_sample=False, eos_token_id=None, use_graph=False)
        tok = generation.generate(m, emb, mask, prompt_alias=alias, **kw)
        assert (cnt.prefills, cnt.chunked) == (1, 0) and tuple(tok.shape) == (B, T)
        rw = generation.rollout_weights(m, rows=B)
        assert rw is generation.rollout_weights(m, rows=16)
        for R in rw:
            assert tuple(R.get("fp8_proj", ())) == ("Wqkv", "Wo", "Wgu", "Wd") and R.get("fp8")
        assert generation.packed_head_fp8(m, rows=B) is not None
        cnt.reset()
        tr32 = []
        f32 = generation.generate(m, emb, mask, prompt_alias=alias, force_tokens=tok, trace_logits=tr32, **kw)
        assert (cnt.prefills, cnt.chunked) == (1, 0)
        monkeypatch.setenv("BRA_FP8_ROWS32", "0")
        cnt.reset()
        tr16 = []
        f16 = generation.generate(m, emb, mask, prompt_alias=alias, force_tokens=tok, trace_logits=tr16, **kw)
        assert cnt.chunked == 1 and cnt.prefills >= 2
        if prompts == 3:
            trb = []
            fb = generation.generate(m, emb[8:24], mask[8:24], prompt_alias=[0] * 8 + [8] * 8, force_tokens=tok[8:24], trace_logits=trb, **kw)
            tr16 = [torch.cat([c[:16], d[8:]], 0) for c, d in zip(tr16, trb)]
            f16 = torch.cat([f16[:16], fb[8:]], 0)
        monkeypatch.delenv("BRA_FP8_ROWS32")
        assert len(tr32) == len(tr16) == T - 1 and tuple(tr32[0].shape) == (B, V)
        for t, (a, c) in enumerate(zip(tr32, tr16)):
            assert torch.equal(a.cpu(), c.cpu()), (t, (a.cpu() != c.cpu()).nonzero()[:4].tolist())
        assert torch.equal(f32, f16)
        assert float(tr32[-1].abs().max()) > 0 and bool(torch.isfinite(tr32[-1]).all())
        if prompts == 4:
            kg = dict(max_new_tokens=40, do_sample=False, eos_token_id=None, prompt_alias=alias)
            g_e = generation.generate(m, emb, mask, use_graph=False, **kg)
            g_g = generation.generate(m, emb, mask, use_graph=True, **kg)
            assert g_e.shape == g_g.shape == (B, 40) and torch.equal(g_e, g_g)
        # the W8A8 prompt pass (default BRA_FP8_PREFILL) over the same weight set
        monkeypatch.delenv("BRA_FP8_PREFILL")
        m.ensure_packed()._rollout = None             # (the cached set was built without the row-major images of the prompt pass)
        assert generation.prefill_fp8_weights(m, 32) is not None
        assert generation.rollout_weights(m, rows=32) is generation.rollout_weights(m, rows=16)
        cnt.reset()
        g8 = generation.generate(m, emb, mask, prompt_alias=alias, **kw)
        assert (cnt.prefills, cnt.chunked) == (2, 0)      # (ONE prompt pass: prefill() re-enters itself once inside eng.use_fp8)
        assert tuple(g8.shape) == (B, T) and int(g8.min()) >= 0 and int(g8.max()) < V
    finally:
        m.rollout_fp8 = False


# ----------------------------------------------------------------------------- 7: ISA (no GPU)
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("c++filt") is None, reason="needs hipcc")
def test_isa_of_the_32_row_fp8_instantiations(tmp_path):
    """every dec_gemm2_kernel<0, NORM, ACT, OUTF32, NW, NL, WIDE = 2, PK = 1, FAST = 1, F8 = 1> of k_decgemm.s: no scratch, at least 24 of
    them, none for the folded norm on 16 waves x 12 chunks, and the first global load within 40 instructions of the compatibility header
    (the bound of test_isa.test_fast_decode_projections_request_weights_before_any_argument_fetch)"""
    from test_isa import _asm, _kernels
    asm = _asm("k_decgemm.hip", tmp_path)
    pat = r"dec_gemm2_kernelILi0ELi(\d)ELi(\d)ELi(\d)ELi(\d+)ELi(\d+)ELi2ELi1ELi1ELi1EEE"
    ks = {n: v for n, v in _kernels(asm).items() if re.search(pat, n)}
    assert len(ks) >= 24, len(ks)
    scratch = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", asm, re.S):
        if m.group(1) in ks:
            scratch[m.group(1)] = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1))
    assert set(scratch) == set(ks)
    forms = set()
    for n, (body, pre) in ks.items():
        norm, act, f32, nw, nl = (int(v) for v in re.search(pat, n).groups())
        forms.add((nw, nl))
        assert not (norm == 2 and nw == 16 and nl == 12), n
        assert norm != 1 and scratch[n] == 0, (n, scratch[n])
        assert pre >= 14, (n, pre)
        start = next(i for i, l in enumerate(body) if l.startswith("s_branch")) + 1
        first_ld = next(i for i, l in enumerate(body) if l.startswith("global_load"))
        assert first_ld - start <= 40, (n, first_ld - start)
    assert forms == set(FORMS.values()), forms
