"""17 .. 32 sequences per GPU in ONE token loop: the 32-row form of the streaming decode projections (k_decgemm.hip, WIDE == 2)
and everything around it (bra_row_sumsq, the sampler's fused embedding gather, generation.generate).

The 32-row form requests every weight fragment once and multiplies it against both 16-row halves of the batch.  Per output
element the K-reduction is the 16-row kernel's own, so the claim these tests rest on is exact: row r of a 32-row launch is
BIT-IDENTICAL to row r computed by the 16-row kernel on the same packed weights and inputs.  The 16-row kernel is the 9 .. 16-row
form (16-column tiles, the rows = 16 weight image); a row block shorter than 9 rows (M = 17 .. 24: rows [16, M)) is therefore
extended to 9 rows with the buffer rows that follow it — 8 rows or fewer select the 8-row kernels, which split K differently and
read another weight image — and only its first M - 16 rows are compared.

Bit-equality alone is self-consistency, so one shape per role is also held to a float64 statement under the bounds
tests/test_kernels.py::test_dec_gemm2_wide_rows uses for the 16-row kernel (4e-3 residual form, 1.5e-2 folded norm / fp32
logits, 2e-2 SwiGLU, 1e-5 statistics).

lm_head with N not a multiple of 16: fragment-packed weights exist only for whole 16-column tiles (bra_dec_pack_weights refuses
anything else) and above 8 rows the norm is only available folded into packed weights, so the ragged last tile of fp32 logits +
tile maxima is exercised in the plain-layout form without norm; the folded packed lm_head runs at N % 16 == 0 as in the model
(Qwen3's V = 151 936 = 16 x 9 496)."""
import os

import pytest
import torch

from bioreason_amd import generation, ops
from bioreason_amd._lib import current_stream, get_lib

GOLD = os.path.join(os.path.dirname(__file__), "golden")
BF = torch.bfloat16
SENT = -77.0                    # sentinel of the rows a launch must not touch
NSS_IN = 64                     # statistics columns of the inputs: 40 non-zero partials per row, folded 8 per lane


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def rnd(*shape, dev, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed * 1000 + sum(shape) + len(shape))
    return (torch.randn(*shape, generator=g) * scale).to(BF).to(dev)


def _gemm(x, M, W, N, K, ss_in=None, norm_w=None, res=None, act=False, out_f32=False, want_ss=False, packed=0, rows_alloc=32):
    """bra_dec_gemm2_packed on rows [0, M) of x into SENT-filled buffers of `rows_alloc` rows -> (out, ss_out | tile maxima | None, rc)"""
    dev = x.device
    out = torch.full((rows_alloc, N // 2 if act else N), SENT, dtype=torch.float32 if out_f32 else BF, device=dev)
    nss_out = ((N + 15) // 16 + 31) // 32 * 32
    sso = torch.full((rows_alloc, nss_out), SENT, dtype=torch.float32, device=dev) if want_ss else None
    rc = get_lib().call_rc("bra_dec_gemm2_packed", x, x.stride(0), ss_in, ss_in.shape[1] if ss_in is not None else 0, norm_w, 1e-6,
                           W, W.stride(0), res, res.stride(0) if res is not None else 0, out, out.stride(0), sso,
                           nss_out if want_ss else 0, M, N, K, int(act), int(out_f32), int(packed), current_stream(x))
    return out, sso, rc


def _stats(x, dev):
    """[32, NSS_IN] partial sums of squares of the 32 rows of x: 40 positive partials per row that add up to the row's sum"""
    g = torch.Generator().manual_seed(11)
    split = torch.softmax(torch.randn(32, 40, generator=g), -1)
    ss = torch.zeros(32, NSS_IN)
    ss[:, :40] = (x.float().cpu() ** 2).sum(1, keepdim=True) * split
    return ss.to(dev)


# K of every (waves, chunks) instantiation of the 9 .. 32-row forms (dg2_waves_and_chunks, 16-column tiles of 32 k):
#   FAST (K == NW * NL * 32):  512 4x4   1024 4x8   1536 4x12   2048 8x8 (Qwen3-1.7B hidden / q width)   2560 8x10 (4B hidden)
#                              3072 8x12   4096 16x8 (4B q width)   6144 16x12 (1.7B intermediate)
#   packed, one clamped round: 256 4x4   768 4x8   1440 4x12   (8x8 / 16x8 have no such K)
#                              2336 8x10   2848 8x12   5664 16x12: refused at 32 rows (BRA_ERR_UNSUPPORTED), as is the plain layout
#                              at the K of the 8x10 / 8x12 / 16x8 / 16x12 forms — asserted as such
#   multi-round loop (no folded norm there): 2304 8x8 x 2 rounds   9728 16x8 x 3 rounds (4B intermediate; packed only)
# and the (N, K) of tests/test_kernels.py::test_dec_gemm2_wide_rows where the emulator can afford them
FAST_K = [512, 1024, 1536, 2048, 2560, 3072, 4096, 6144]
SLOW_K = [256, 768, 1440, 2336, 2848, 5664]
MULTI_K = [2304, 9728]
SHAPES = ([(48, k) for k in FAST_K + SLOW_K + MULTI_K] + [(256, 256), (96, 512)]
          + [pytest.param(2048, 2048, marks=pytest.mark.gpu), pytest.param(2048, 6144, marks=pytest.mark.gpu),
             pytest.param(4096, 2048, marks=pytest.mark.gpu)])
F64_SHAPE = (96, 512)


def _single_round(K):
    return K not in MULTI_K


@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("M", [17, 24, 31, 32])
def test_rows32_projection_rows_equal_the_16_row_kernel(backend, M, N, K):
    if backend.type == "cpu" and N * K > 3e6:
        pytest.skip("emulator: large shape covered on the GPU")
    dev = backend
    mb = max(M - 16, 9)                        # rows of the second 16-row call (see the module docstring)
    x, W = rnd(32, K, dev=dev, seed=1), rnd(N, K, dev=dev, scale=K ** -0.5, seed=2)
    nw = (1 + 0.1 * rnd(K, dev=dev, seed=3).float()).to(BF)
    res = rnd(32, N, dev=dev, seed=4)
    ss = _stats(x, dev)
    Wp = ops.dec_pack_weights(W, rows=16)                              # o / down
    Wf = ops.dec_pack_weights(W, norm_w=nw, rows=16)                   # qkv
    Wa = ops.dec_pack_weights(W, act=True, norm_w=nw, rows=16)         # gate / up
    Wh = ops.dec_pack_weights(W, out_f32=True, norm_w=nw, rows=16)     # lm_head
    Nr = N - 5                                                         # ragged lm_head (plain layout, no norm)
    roles = [("o/down", dict(W=Wp, N=N, res=True, want_ss=True, packed=1)),
             ("o/down plain", dict(W=W, N=N, res=True, want_ss=True, packed=0)),
             ("lm_head ragged plain", dict(W=W, N=Nr, out_f32=True, want_ss=True, packed=0))]
    if _single_round(K):
        roles += [("qkv", dict(W=Wf, N=N, norm=True, packed=3)),
                  ("gate/up", dict(W=Wa, N=N, norm=True, act=True, packed=3)),
                  ("lm_head", dict(W=Wh, N=N, norm=True, out_f32=True, want_ss=True, packed=3))]
    xd, Wd, nwd = x.double().cpu(), W.double().cpu(), nw.double().cpu()
    xn = xd * torch.rsqrt((xd * xd).mean(1, keepdim=True) + 1e-6) * nwd
    for name, r in roles:
        n = r["N"]

        def run(lo, m, rows_alloc):
            return _gemm(x[lo:], m, r["W"], n, K, ss_in=ss[lo:] if r.get("norm") else None, norm_w=nw if r.get("norm") else None,
                         res=res[lo:] if r.get("res") else None, act=r.get("act", False), out_f32=r.get("out_f32", False),
                         want_ss=r.get("want_ss", False), packed=r["packed"], rows_alloc=rows_alloc)
        y, s, rc = run(0, M, 32)
        # the library has no 32-row kernel for some (waves, chunks) forms outside the fast one — those that would not hold both row
        # halves in registers (generation.rows32_form_exists states launch_dg2's rule): exactly those are refused, and untouched
        if not generation.rows32_form_exists(K, normed=bool(r.get("norm")), packed=bool(r["packed"])):
            assert rc == -2 and bool((y.float() == SENT).all()), (name, rc)
            continue
        assert rc == 0, (name, rc)
        ya, sa, rca = run(0, 16, 16)
        yb, sb, rcb = run(16, mb, 16)
        assert rca == 0 and rcb == 0, name
        assert torch.equal(y[:16], ya), name                                   # rows 0 .. 15
        assert torch.equal(y[16:M], yb[:M - 16]), name                         # rows 16 .. M - 1
        assert bool((y[M:].float() == SENT).all()), name                       # rows past M: never stored
        if s is not None:
            nt = (n + 15) // 16
            assert torch.equal(s[:16, :nt], sa[:, :nt]) and torch.equal(s[16:M, :nt], sb[:M - 16, :nt]), name
            assert bool((s[M:] == SENT).all()) and bool((s[:, nt:] == SENT).all()), name
        if (N, K) != F64_SHAPE:
            continue
        # float64 statement (the 16-row kernel's bounds, test_dec_gemm2_wide_rows)
        yd = y[:M].double().cpu()
        if name.startswith("o/down"):
            want = ((xd[:M] @ Wd.T).to(BF).double() + res[:M].double().cpu()).to(BF)
            assert rel(yd, want) < 4e-3, name
            assert rel(s[:M, :N // 16].sum(1), (yd ** 2).sum(1)) < 1e-5, name
        elif name == "qkv":
            assert rel(yd, xn[:M] @ Wd.T) < 1.5e-2, name
        elif name == "gate/up":
            r3 = (xn[:M] @ Wd.T).view(M, N // 16, 2, 8)
            g, u = r3[:, :, 0].reshape(M, -1), r3[:, :, 1].reshape(M, -1)
            assert rel(yd, torch.nn.functional.silu(g) * u) < 2e-2, name
        else:
            ref = (xn[:M] @ Wd.T) if name == "lm_head" else (xd[:M] @ Wd[:n].T)
            assert rel(yd, ref) < 1.5e-2, name
            tm = torch.nn.functional.pad(yd, (0, (-n) % 16), value=-float("inf")).view(M, -1, 16).amax(-1)
            assert torch.equal(s[:M, :(n + 15) // 16].double().cpu(), tm), name            # maxima of exactly the logits stored


def test_rows32_projection_refuses_what_it_does_not_stream(backend):
    """above 16 rows: an unfolded norm (row-major or packed without the fold) is BRA_ERR_UNSUPPORTED (the host falls back to
    chunks), more than 32 rows an argument error"""
    dev = backend
    N, K = 48, 512
    x, W = rnd(32, K, dev=dev, seed=1), rnd(N, K, dev=dev, scale=K ** -0.5, seed=2)
    nw = (1 + 0.1 * rnd(K, dev=dev, seed=3).float()).to(BF)
    ss = _stats(x, dev)
    assert _gemm(x, 17, W, N, K, ss_in=ss, norm_w=nw)[2] == -2
    assert _gemm(x, 17, ops.dec_pack_weights(W, rows=16), N, K, ss_in=ss, norm_w=nw, packed=1)[2] == -2
    x40 = rnd(40, K, dev=dev, seed=5)
    with pytest.raises(RuntimeError):
        _gemm(x40, 33, W, N, K, rows_alloc=40)


@pytest.mark.parametrize("M", [17, 32])
def test_row_sumsq_and_sampler_gather_up_to_32_rows(backend, M):
    """bra_row_sumsq and the drawing wave's x = E[token] + row statistic at 17 and 32 rows against the <= 16-row calls on the row
    blocks: equal, and nothing written past row M"""
    dev = backend
    K = 264
    x = rnd(M, K, dev=dev, seed=7)
    ss = ops.row_sumsq(x, 32)
    assert ss.shape == (32, 32)
    assert torch.equal(ss[:16], ops.row_sumsq(x[:16], 32)) and torch.equal(ss[16:M], ops.row_sumsq(x[16:M], 32)[:M - 16])
    assert float(ss[M:].abs().max()) == 0.0 if M < 32 else True
    xd = x.double().cpu()
    assert rel(ss[:M, 0], (xd * xd).sum(1)) < 1e-5 and float(ss[:, 1:].abs().max()) == 0.0

    V, H = 4608, 64
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(M, V, generator=g).to(dev)
    E = rnd(V, H, dev=dev, seed=8)
    step = torch.zeros(1, dtype=torch.int32, device=dev)

    def draw(lo, hi, rows_ss, tiles):
        n = hi - lo
        xo = torch.full((32, H), SENT, dtype=BF, device=dev)
        so = torch.full((rows_ss, 32), 7.0, device=dev)
        out = torch.empty(n, dtype=torch.int32, device=dev)
        lg = logits[lo:hi].contiguous()
        if tiles:
            ops.sample_tiles(lg, ops.tile_max(lg), 1.0, 0, 1.0, False, 0, step, None, 0, out, embed=(E, xo, so))
        else:
            ops.sample(lg, 1.0, 0, 1.0, False, 0, step, None, 0, out, embed=(E, xo, so))
        return out, xo, so
    for tiles in (False, True):
        out, xo, so = draw(0, M, 32, tiles)
        assert out.tolist() == logits.argmax(-1).tolist()
        assert torch.equal(xo[:M].cpu(), E[out.long()].cpu()) and bool((xo[M:].float() == SENT).all())
        assert float(so[:M, 1:].abs().max()) == 0.0 and bool((so[M:] == 7.0).all())
        oa, xa, sa = draw(0, 16, 16, tiles)
        ob, xb, sb = draw(16, M, 16, tiles)
        assert torch.equal(out[:16], oa) and torch.equal(out[16:], ob)
        assert torch.equal(xo[:16], xa[:16]) and torch.equal(xo[16:M], xb[:M - 16])
        assert torch.equal(so[:16], sa) and torch.equal(so[16:M], sb[:M - 16])


# ----------------------------------------------------------------------------- generate(): one prefill, one token loop
def _tiny_b(dev):
    from test_model_parity import build, to_dev
    fix = torch.load(os.path.join(GOLD, "tiny_b.pt"), weights_only=False)
    return fix, build(fix, dev, True), to_dev(fix["batch"], dev)


BATCHES = {"2x10": ([0] * 10 + [1] * 10, [0] * 10 + [10] * 10),
           "3x8": ([0] * 8 + [1] * 8 + [2] * 8, [0] * 8 + [8] * 8 + [16] * 8),
           "4x8": ([0] * 8 + [1] * 8 + [2] * 8 + [0] * 8, [0] * 8 + [8] * 8 + [16] * 8 + [24] * 8),
           "32 plain": ([0] * 11 + [1] * 11 + [2] * 10, None)}


class _Counter:
    """counts the prefills and the entries into the row-chunk path of generation.generate"""

    def __init__(self, monkeypatch):
        self.prefills, self.chunked = 0, 0
        real_prefill, real_chunks = generation.prefill, generation._generate_in_row_chunks

        def prefill(*a, **k):
            self.prefills += 1
            return real_prefill(*a, **k)

        def chunks(*a, **k):
            self.chunked += 1
            return real_chunks(*a, **k)
        monkeypatch.setattr(generation, "prefill", prefill)
        monkeypatch.setattr(generation, "_generate_in_row_chunks", chunks)

    def reset(self):
        self.prefills, self.chunked = 0, 0


def _inputs(b, rows, alias):
    ids, mask = b["input_ids"][rows], b["attention_mask"][rows]
    kw = {"input_ids": ids, "attention_mask": mask, "dna_tokenized": {k: v[rows] for k, v in b["dna_tokenized"].items()},
          "batch_idx_map": list(range(len(rows)))}
    if alias is not None:
        kw["prompt_alias"] = alias
    return kw


@pytest.mark.parametrize("batch", list(BATCHES))
def test_one_token_loop_decodes_what_the_row_chunks_decode(backend, monkeypatch, batch):
    """17 .. 32 rows: the one-loop path (BRA_DEC_ROWS32=1) runs ONE prefill and never enters the row-chunk path; its teacher-forced logits are bit-equal
    to those of the 16-row chunks (BRA_DEC_ROWS32=0) at every step and its free greedy tokens are the same.

    3 x 8 rows is the one batch whose chunked form ends in a chunk of EIGHT rows, (0, 16) + (16, 24), and eight rows or fewer run the
    8-row kernels (diagonal tiles for o / down: K reduced as two halves, another weight image), which round differently from the
    16-row kernel the 32-row form is bit-identical to — seen on the emulator: logits of rows 16 .. 23 differ from the 8-row
    chunk's by about 5e-3 (bf16 rounding of values of order 1 - 10) from the third step on; rows 0 .. 15 are equal.  For those eight rows the bit-for-bit reference is therefore the
    16-row loop over groups 2 + 3 (rows 8 .. 23), whose rows 8 .. 15 are the same sequences through the 16-row kernels; against the
    8-row chunk itself their teacher-forced choices may differ in near-ties only (the bound of
    test_model_parity.py::test_decode_with_more_than_sixteen_sequences).  Every other row of every batch is held to the chunks."""
    fix, m, b = _tiny_b(backend)
    cfg = fix["config"]
    rows, alias = BATCHES[batch]
    inp = _inputs(b, rows, alias)
    B, T = len(rows), cfg["gen_tokens"]
    want = fix["fp32_lora"]["greedy_ids"][rows].to(backend)
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
    monkeypatch.setenv("BRA_DEC_ROWS32", "0")
    cnt.reset()
    tr16 = []
    f16 = m.generate(**inp, trace_logits=tr16, **forced)
    assert cnt.chunked == 1 and cnt.prefills >= 2                    # the switch restores the 16-row chunks
    g16 = m.generate(**inp, **free)
    assert f32.shape == f16.shape == g32.shape == g16.shape == (B, T)
    assert len(tr32) == len(tr16) == T - 1 and tr32[0].shape == (B, cfg["text"]["vocab_size"])
    if batch == "3x8":
        # rows 16 .. 23 through the 16-row kernels: the 16-row loop over rows 8 .. 23 (see the docstring)
        inp_b = _inputs(b, rows[8:24], [0] * 8 + [8] * 8)
        trb = []
        fb = m.generate(**inp_b, trace_logits=trb, **dict(forced, force_tokens=want[8:24]))
        gb = m.generate(**inp_b, **free)
        scores = fix["fp32_lora"]["greedy_scores"][rows]
        for bi, t in (f32[16:] != f16[16:]).nonzero().tolist():            # against the 8-row chunk: near-ties only
            a, c = int(f32[16 + bi, t]), int(f16[16 + bi, t])
            assert abs((scores[16 + bi, t, a] - scores[16 + bi, t, c]).item()) < 0.02 * scores[16 + bi, t].abs().max().item() + 0.05
        assert int((f32[16:] != f16[16:]).sum()) <= 6
        tr16 = [torch.cat([c[:16], d[8:]], 0) for c, d in zip(tr16, trb)]
        f16, g16 = torch.cat([f16[:16], fb[8:]], 0), torch.cat([g16[:16], gb[8:]], 0)
    for t, (a, c) in enumerate(zip(tr32, tr16)):
        assert torch.equal(a.cpu(), c.cpu()), (t, (a.cpu() != c.cpu()).nonzero()[:4].tolist())
    assert torch.equal(f32, f16) and torch.equal(g32, g16)


@pytest.mark.gpu
def test_one_token_loop_under_graph_replay(backend, monkeypatch):
    if backend.type == "cpu":
        pytest.skip("graph capture needs a GPU stream")
    fix, m, b = _tiny_b(backend)
    monkeypatch.setenv("BRA_DEC_ROWS32", "1")
    cnt = _Counter(monkeypatch)
    for batch in ("3x8", "32 plain"):
        inp = _inputs(b, *BATCHES[batch])
        kw = dict(max_new_tokens=40, do_sample=False, eos_token_id=None)
        g_e = m.generate(**inp, use_graph=False, **kw)
        g_g = m.generate(**inp, use_graph=True, **kw)
        assert g_e.shape == g_g.shape and torch.equal(g_e, g_g)
    assert (cnt.prefills, cnt.chunked) == (4, 0)


def test_sampling_with_32_rows(backend, monkeypatch):
    """do_sample at 32 rows: reproducible, inside the vocabulary, and the stream of a row does not depend on B — rows 0 .. 15 draw
    what a 16-row call on those rows draws with the same seed"""
    fix, m, b = _tiny_b(backend)
    monkeypatch.setenv("BRA_DEC_ROWS32", "1")
    rows, alias = BATCHES["4x8"]
    kw = dict(max_new_tokens=fix["config"]["gen_tokens"], do_sample=True, temperature=0.6, top_k=20, top_p=0.95, eos_token_id=None,
              seed=5, use_graph=False)
    s1 = m.generate(**_inputs(b, rows, alias), **kw)
    s2 = m.generate(**_inputs(b, rows, alias), **kw)
    assert s1.shape == (32, fix["config"]["gen_tokens"]) and torch.equal(s1, s2)
    assert int(s1.min()) >= 0 and int(s1.max()) < fix["config"]["text"]["vocab_size"]
    s16 = m.generate(**_inputs(b, rows[:16], alias[:16]), **kw)
    assert torch.equal(s1[:16], s16)


def test_more_than_32_rows_run_as_chunks_of_32(backend, monkeypatch):
    """40 rows without alias: (0, 32), (32, 40); teacher-forced choices are those of the op-by-op decode up to near-ties (the
    tolerance of test_model_parity.py::test_decode_with_more_than_sixteen_sequences)"""
    from bioreason_amd.generation import _row_chunks
    assert _row_chunks(40, None, max_rows=32) == [(0, 32), (32, 40)]
    assert _row_chunks(40, None) == [(0, 16), (16, 32), (32, 40)]                            # the default is unchanged
    assert _row_chunks(48, [0] * 24 + [24] * 24, max_rows=32) == [(0, 24), (24, 48)]         # whole groups where they fit
    assert _row_chunks(40, [0] * 40, max_rows=32) == [(0, 32), (32, 40)]
    fix, m, b = _tiny_b(backend)
    cfg = fix["config"]
    monkeypatch.setenv("BRA_DEC_ROWS32", "1")
    rows = [0] * 14 + [1] * 13 + [2] * 13
    inp = _inputs(b, rows, None)
    want = fix["fp32_lora"]["greedy_ids"][rows].to(backend)
    scores = fix["fp32_lora"]["greedy_scores"][rows]
    seen = []
    real = generation._row_chunks
    monkeypatch.setattr(generation, "_row_chunks", lambda *a, **k: seen.append(real(*a, **k)) or seen[-1])
    kw = dict(max_new_tokens=cfg["gen_tokens"], do_sample=False, eos_token_id=None, force_tokens=want)
    g_s = m.generate(**inp, **kw)
    assert seen == [[(0, 32), (32, 40)]]
    g_u = m.generate(**inp, decode_impl="unfused", **kw)
    assert g_s.shape == g_u.shape == (40, cfg["gen_tokens"])
    diff = (g_u != g_s).nonzero().tolist()
    for bi, t in diff:
        a, c = int(g_u[bi, t]), int(g_s[bi, t])
        assert abs((scores[bi, t, a] - scores[bi, t, c]).item()) < 0.02 * scores[bi, t].abs().max().item() + 0.05
    assert len(diff) <= 6
