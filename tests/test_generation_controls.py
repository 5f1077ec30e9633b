"""repetition_penalty, min_new_tokens and min_p in the token loop (bra_logits_process in front of the samplers, min_p inside them).

The yardstick everywhere is the installed `transformers.generation.logits_process` classes run on the CPU (fp32 where bit-equality
is asked, float64 for probabilities): RepetitionPenaltyLogitsProcessor -> MinNewTokensLengthLogitsProcessor -> TemperatureLogitsWarper
-> TopKLogitsWarper -> TopPLogitsWarper -> MinPLogitsWarper, the order of GenerationMixin._get_logits_processor.  The history the
penalty runs over is the GENERATED tokens only: `test_hf_penalises_generated_tokens_only` pins that this is what HF does for a
generate() call with inputs_embeds and no input_ids, which is how the reference calls it.

min_new_tokens writes -inf, as HF does: the samplers' candidate keys order -inf below every finite value and exp(-inf) = 0, so a
banned id is outside the support and never the arg-max."""
import os
from types import SimpleNamespace

import pytest
import torch
from transformers.generation.logits_process import (MinNewTokensLengthLogitsProcessor, MinPLogitsWarper,
                                                    RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper, TopKLogitsWarper,
                                                    TopPLogitsWarper)

from bioreason_amd import generation, ops
from bioreason_amd._lib import KernelError

GOLD = os.path.join(os.path.dirname(__file__), "golden")
SENT = -77.0


# --------------------------------------------------------------------------------------------------------------- HF yardsticks
def hf_process(scores, hist, penalty, min_new, eos_ids):
    """RepetitionPenalty -> MinNewTokensLength of the installed transformers on CPU scores [B, V] with history `hist` [B, t] (long)"""
    out = scores.clone()
    if penalty != 1.0 and hist.shape[1] > 0:
        out = RepetitionPenaltyLogitsProcessor(float(penalty))(hist, out)
    eos_ids = [e for e in eos_ids if e >= 0]
    if min_new > 0 and eos_ids:
        out = MinNewTokensLengthLogitsProcessor(0, int(min_new), eos_ids, device="cpu")(hist, out.clone())
    return out


def hf_warp_probs(logits, T, top_k, top_p, min_p):
    """float64 probabilities of Temperature -> TopK -> TopP -> MinP (zeros outside the support)"""
    sc = logits.double().clone()
    none = torch.zeros((sc.shape[0], 0), dtype=torch.long)
    sc = TemperatureLogitsWarper(float(T))(none, sc)
    if top_k > 0:
        sc = TopKLogitsWarper(int(top_k))(none, sc)
    if top_p < 1.0:
        sc = TopPLogitsWarper(float(top_p))(none, sc)
    if min_p > 0.0:
        sc = MinPLogitsWarper(float(min_p))(none, sc)
    return torch.softmax(sc, -1)


def ulp_dist(a, b):
    """distance in units of the last place between fp32 tensors of equal sign"""
    ia, ib = a.contiguous().view(torch.int32).long(), b.contiguous().view(torch.int32).long()
    return (ia - ib).abs()


# ----------------------------------------------------------------------------------------------------- 1. semantics pin (CPU)
def test_hf_penalises_generated_tokens_only():
    """HF generate(inputs_embeds=..., repetition_penalty, min_new_tokens) == a loop applying the two processors to the
    generated-only history, != the same loop with the prompt ids in the history (float64: no near-ties between cached and
    uncached forwards)"""
    from oracle.dna_llm_oracle import make_qwen3
    torch.manual_seed(2)
    V, P, T, pen, mn = 64, 32, 12, 1.5, 6
    hf = make_qwen3({"vocab_size": V, "hidden_size": 32, "intermediate_size": 64, "num_hidden_layers": 2, "num_attention_heads": 2,
                     "num_key_value_heads": 1, "head_dim": 16}).double().eval()
    B = 2
    # half of the vocabulary occurs in the prompt: penalising those ids changes the first choice (seed chosen so that it does)
    prompt = torch.stack([torch.randperm(V) for _ in range(B)])[:, :P]
    emb = hf.get_input_embeddings()
    mask = torch.ones(B, P, dtype=torch.long)

    def logits_after(gen):
        ids = torch.cat([prompt, gen], 1)
        with torch.no_grad():
            return hf(inputs_embeds=emb(ids), attention_mask=torch.ones_like(ids)).logits[:, -1]

    eos = int(logits_after(torch.zeros(B, 0, dtype=torch.long))[0].argmax())   # row 0 would stop at once without min_new_tokens
    pad = 0

    def loop(with_prompt):
        gen = torch.zeros(B, 0, dtype=torch.long)
        unfinished = torch.ones(B, dtype=torch.bool)
        rp = RepetitionPenaltyLogitsProcessor(pen)
        ml = MinNewTokensLengthLogitsProcessor(P if with_prompt else 0, mn, [eos], device="cpu")
        for _ in range(T):
            raw = logits_after(gen)
            hist = torch.cat([prompt, gen], 1) if with_prompt else gen
            sc = ml(hist, rp(hist, raw.clone()) if hist.shape[1] else raw.clone())
            nxt = sc.argmax(-1)
            nxt = torch.where(unfinished, nxt, torch.full_like(nxt, pad))
            gen = torch.cat([gen, nxt[:, None]], 1)
            unfinished &= nxt != eos
            if not unfinished.any():
                break
        return gen

    with torch.no_grad():
        out = hf.generate(inputs_embeds=emb(prompt), attention_mask=mask, max_new_tokens=T, do_sample=False, repetition_penalty=pen,
                          min_new_tokens=mn, eos_token_id=eos, pad_token_id=pad)
    own, with_prompt = loop(False), loop(True)
    assert out.shape == own.shape and torch.equal(out, own)
    assert not (with_prompt.shape == out.shape and torch.equal(out, with_prompt))
    assert not bool((out[:, :mn] == eos).any())


# ------------------------------------------------------------------------------------- 2. ops.logits_process vs the HF processors
LP_B, LP_V = 3, 5000                       # >= 4096 (two-stage sampler), not a multiple of 16 (ragged last tile: columns 4992 .. 4999)
LP_EOS = (4990, 17)                        # the second one shares tile 1 with nothing of the history; the first sits next to the ragged tile


def _lp_inputs():
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(LP_B, LP_V, generator=g) * 3.0
    # columns 0 .. 4 of every history: a duplicate, two ids of one 16-column tile (7, 8), id 0, an id of the ragged tile — with
    # logits of both signs, the ragged one the maximum of its tile (the penalty lowers that tile's maximum)
    logits[:, 7], logits[:, 8], logits[:, 0], logits[:, 4995] = 2.5, -1.25, -0.3, 14.0
    logits[1, 7], logits[2, 4995] = -2.5, -0.75
    pool = torch.randint(0, LP_V, (40,), generator=g)                     # 295 entries over 40 ids: most of them duplicated
    hist = pool[torch.randint(0, 40, (LP_B, 8300), generator=g)]
    hist[:, :5] = torch.tensor([7, 7, 8, 0, 4995])
    hist[2, 1] = 4999                                                      # the last column of the vocabulary
    return logits, hist.to(torch.int32)


@pytest.mark.parametrize("step_kind", ["device_word", "int"])
@pytest.mark.parametrize("t", [0, 1, 5, 300])
def test_logits_process_matches_hf_processors(backend, t, step_kind):
    dev = backend
    logits, hist = _lp_inputs()
    hist_d = hist[:, :320].contiguous().to(dev)
    step = torch.tensor([t], dtype=torch.int32, device=dev) if step_kind == "device_word" else t
    cases = [(pen, mn, eos) for pen in (1.3, 0.8)
             for mn, eos in ((0, (-1, -1)), (t + 1, (LP_EOS[0], -1)), (t + 3, LP_EOS), (t, LP_EOS))]
    cases += [(1.0, t + 1, LP_EOS), (1.0, 0, LP_EOS)]                      # min_new_tokens alone; everything off (no launch)
    for pen, mn, eos in cases:
        want = hf_process(logits, hist[:, :t].long(), pen, mn, eos)
        buf = torch.full((LP_B + 2, LP_V), SENT, dtype=torch.float32)
        buf[:LP_B] = logits
        buf = buf.to(dev)
        lg = buf[:LP_B]
        tbuf = torch.full((LP_B + 2, (LP_V + 15) // 16), SENT, dtype=torch.float32, device=dev)
        tm = tbuf[:LP_B]
        ops.tile_max(lg, tm)
        ops.logits_process(lg, hist_d, step, pen, mn, eos[0], eos[1], None, tm)
        got = lg.cpu()
        banned = torch.zeros(LP_B, LP_V, dtype=torch.bool)
        if t < mn:
            for e in eos:
                if e >= 0:
                    banned[:, e] = True
        seen = torch.zeros(LP_B, LP_V, dtype=torch.bool)
        if pen != 1.0 and t > 0:
            seen.scatter_(1, hist[:, :t].long(), True)
        seen &= ~banned
        same = ~seen & ~banned
        key = (t, pen, mn, eos)
        assert torch.equal(got[same].view(torch.int32), logits[same].view(torch.int32)), key            # untouched: bit-equal
        assert torch.equal(want[same].view(torch.int32), logits[same].view(torch.int32)), key            # (and HF agrees they are)
        mul = seen & (logits < 0)
        assert torch.equal(got[mul].view(torch.int32), want[mul].view(torch.int32)), key                 # l * penalty: bit-equal
        div = seen & ~(logits < 0)
        if t >= 5 and pen != 1.0:
            assert bool(mul[0].any()) and bool(div[0].any()) and int(seen[0].sum()) < t
        assert int(ulp_dist(got[div], want[div]).max()) <= 2 if bool(div.any()) else True, key           # l / penalty: 2 ulp
        assert bool((got[banned] == float("-inf")).all()) and bool((want[banned] == float("-inf")).all()), key
        assert torch.equal(tm.cpu().view(torch.int32), ops.tile_max(lg).cpu().view(torch.int32)), key    # maxima of what is stored
        assert bool((buf[LP_B:] == SENT).all()) and bool((tbuf[LP_B:] == SENT).all()), key                # rows past B
    # a finished row is left alone; the others are processed
    lg = logits.clone().to(dev)
    fin = torch.tensor([0, 1, 0], dtype=torch.uint8, device=dev)
    ops.logits_process(lg, hist_d, step, 1.3, t + 1, LP_EOS[0], -1, fin, None)
    assert torch.equal(lg[1].cpu(), logits[1]) and bool((lg[0].cpu() != logits[0]).any())


def test_logits_process_refuses_a_history_beyond_its_staging(backend):
    """the penalty stages one logit per history entry in LDS (8192 entries): 8193 is BRA_ERR_UNSUPPORTED and nothing is written —
    as an int and as a device word over a history that wide; 8192 entries are served; argument errors are argument errors"""
    dev = backend
    logits, hist = _lp_inputs()
    lg = logits.clone().to(dev)
    tm = ops.tile_max(lg)
    tm0 = tm.clone()
    for cols, step in ((8193, 8193), (8193, torch.tensor([3], dtype=torch.int32, device=dev))):
        with pytest.raises(KernelError) as ei:
            ops.logits_process(lg, hist[:, :cols].contiguous().to(dev), step, 1.3, 0, -1, -1, None, tm)
        assert ei.value.status == -2
        assert torch.equal(lg.cpu(), logits) and torch.equal(tm, tm0)
    h = hist[:, :8192].contiguous()
    ops.logits_process(lg, h.to(dev), 8192, 1.3, 0, -1, -1, None, tm)
    want = hf_process(logits, h.long(), 1.3, 0, ())
    assert int(ulp_dist(lg.cpu(), want).max()) <= 2 and torch.equal(tm, ops.tile_max(lg))
    with pytest.raises(KernelError) as ei:
        ops.logits_process(lg, h.to(dev), 5, 0.0, 0, -1, -1, None, None)                 # penalty must be > 0
    assert ei.value.status == -1
    with pytest.raises(KernelError) as ei:
        ops.logits_process(lg, h[:, :4].contiguous().to(dev), 5, 1.3, 0, -1, -1, None, None)   # a step past the history handed in
    assert ei.value.status == -1
    ops.logits_process(lg[:0], h[:0].to(dev), 5, 1.3, 0, -1, -1, None, None)             # B == 0


# ----------------------------------------------------------------------------------------------------- 3. min_p in the samplers
MP_T, MP_K, MP_P = 0.6, 20, 0.95
MP_FULL_T, MP_FULL_P = 0.7, 0.9
MP_SMALL = 1e-9


def _mp_logits(V, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(3, V, generator=g) * 2.0
    logits[0] *= 0.2                                  # flat row
    logits[1, 123] += 6.0                             # peaked row
    return logits                                     # row 2: ordinary


def _assert_clear_of_min_p_boundary(logits, T, top_k, top_p, min_ps):
    """no survivor of top-k / top-p has a probability ratio to the top within 1e-3 relative of a tested min_p (boundary rounding
    stays out of the comparison), and the small value removes nothing"""
    base = hf_warp_probs(logits, T, top_k, top_p, 0.0)
    ratio = base / base.max(-1, keepdim=True)[0]
    sup = base > 0
    for mp in min_ps:
        assert bool(((ratio[sup] / mp - 1.0).abs() > 1e-3).all()), mp
    assert bool((ratio[sup] > 1e3 * MP_SMALL).all())


@pytest.mark.parametrize("kind", ["sample", "sample_tiles", "sample_full"])
def test_min_p_in_the_samplers(backend, kind):
    dev = backend
    on_gpu = dev.type == "cuda"
    full = kind == "sample_full"
    # the general kernel keeps hundreds of survivors per row (top_k = 0): at V = 6000 their probability ratios lie closer together
    # than the 1e-3 clearance around min_p asked for below, so its rows are 1500 wide (two indices per thread of its 1024)
    V, seed = (1500, 9) if full else (6000, 3)        # seeds chosen so that the clearance assertion holds
    T, k, p = (MP_FULL_T, 0, MP_FULL_P) if full else (MP_T, MP_K, MP_P)
    logits = _mp_logits(V, seed)
    _assert_clear_of_min_p_boundary(logits, T, k, p, (0.05, 0.3))
    R, steps = (40, 100) if on_gpu else (1, 10)       # 4000 draws per row on the GPU; the emulator run checks the support
    B = 3 * R
    dl = logits.repeat(R, 1).contiguous().to(dev)     # launch row r draws for row r % 3 (the draw stream depends on the row index)
    tmax = ops.tile_max(dl) if kind == "sample_tiles" else None
    ws = torch.empty((2 * B * 64 * MP_K,), dtype=torch.float32, device=dev)
    step_t = torch.zeros(1, dtype=torch.int32, device=dev)

    def run(min_p):
        toks = torch.full((B, steps), -1, dtype=torch.int32, device=dev)
        lps = torch.zeros((steps, B), dtype=torch.float32, device=dev)
        out = torch.empty(B, dtype=torch.int32, device=dev)
        for s in range(steps):
            if kind == "sample":
                step_t.fill_(s)
                ops.sample(dl, T, k, p, True, 99, step_t, None, 0, out, out_logp=lps[s], tokens_out=toks, ws=ws, min_p=min_p)
            elif kind == "sample_tiles":
                ops.sample_tiles(dl, tmax, T, k, p, True, 99, s, None, 0, out, out_logp=lps[s], tokens_out=toks, ws=ws, min_p=min_p)
            else:
                ops.sample_full(dl, T, k, p, 99, s, None, 0, out, out_logp=lps[s], tokens_out=toks, min_p=min_p)
        return toks.cpu().long(), lps.cpu().double().t().contiguous()          # [B, steps] both

    def logp_dev(toks, lps, want):
        pr = want[torch.arange(B) % 3][torch.arange(B)[:, None], toks]
        assert bool((pr > 0).all()), "draw outside the HF warpers' support"
        return float((lps - pr.log()).abs().max())

    t0, l0 = run(0.0)
    base_dev = logp_dev(t0, l0, hf_warp_probs(logits, T, k, p, 0.0))           # the path as it stands
    ts, ls = run(MP_SMALL)                                                      # removes nothing: the same draws, bit for bit
    assert torch.equal(ts, t0) and torch.equal(ls, l0)
    for mp in (0.05, 0.3):
        want = hf_warp_probs(logits, T, k, p, mp)
        assert int((want > 0).sum()) < int((hf_warp_probs(logits, T, k, p, 0.0) > 0).sum())      # the filter bites
        toks, lps = run(mp)
        d = logp_dev(toks, lps, want)
        print(f"{kind} min_p={mp}: |out_logp - log p_HF| max {d:.3e} (min_p = 0: {base_dev:.3e})")
        assert d <= 2.0 * base_dev, (kind, mp, d, base_dev)
        if not on_gpu:
            continue
        n = R * steps
        for b in range(3):
            counts = torch.bincount(toks[b::3].reshape(-1), minlength=V).double()
            sup = want[b] > 0
            e = want[b][sup] * n
            chi2 = (((counts[sup] - e) ** 2) / e).sum().item()
            dof = int(sup.sum()) - 1
            # the bound of test_kernels.py::test_sampler_distribution_matches_oracle_warpers
            assert chi2 <= dof + 5.0 * (2.0 * max(dof, 1)) ** 0.5 + 5.0, (kind, mp, b, chi2, dof)


# ------------------------------------------------------------------------------------------- 4. end to end on the tiny_b fixture
PEN, MIN_NEW = 5.0, 5                  # (the fixture's top logit is 2.3 .. 4.2 x its runner-up: a smaller penalty changes no arg-max)


def _tiny_b(dev):
    from test_model_parity import build, to_dev
    fix = torch.load(os.path.join(GOLD, "tiny_b.pt"), weights_only=False)
    return fix, build(fix, dev, True), to_dev(fix["batch"], dev)


def _inputs(b, rows, alias=None):
    kw = {"input_ids": b["input_ids"][rows], "attention_mask": b["attention_mask"][rows],
          "dna_tokenized": {k: v[rows] for k, v in b["dna_tokenized"].items()}, "batch_idx_map": list(range(len(rows)))}
    if alias is not None:
        kw["prompt_alias"] = alias
    return kw


def _eos_for(fix):
    """two stop ids the fixture's model actually reaches for: the greedy token of row 0 and of row 1"""
    g = fix["fp32_lora"]["greedy_ids"]
    return [int(g[0, 0]), int(g[1, 0])]


def _expect_forced(trace, force, eos, pen, mn, pad):
    """per step t >= 1: the arg-max of the HF processors over the traced raw logits tr[t - 1] with history force[:, :t] -> (tokens
    [B, T] with column 0 unset, raw arg-max [B, T], near-tie mask [B, T]); a row that drew an EOS id emits pad from then on"""
    B, T = force.shape
    want = torch.full((B, T), -1, dtype=torch.long)
    raw_am = torch.full((B, T), -1, dtype=torch.long)
    tie = torch.zeros((B, T), dtype=torch.bool)
    for t in range(1, T):
        raw = trace[t - 1].float().cpu()
        sc = hf_process(raw, force[:, :t].long().cpu(), pen, mn, eos)
        top2 = sc.topk(2, -1)[0]
        tie[:, t] = ulp_dist(top2[:, 0], top2[:, 1]) <= 4
        want[:, t], raw_am[:, t] = sc.argmax(-1), raw.argmax(-1)
    return want, raw_am, tie


def _check_forced(out, trace, force, eos, pen, mn, pad):
    out = out.cpu()
    want, raw_am, tie = _expect_forced(trace, force, eos, pen, mn, pad)
    B, T = force.shape
    assert out.shape == (B, T) and len(trace) == T - 1
    is_eos = torch.zeros_like(out, dtype=torch.bool)
    for e in eos:
        is_eos |= out == e
    assert not bool(is_eos[:, :mn].any())                                   # no EOS id among the first min_new_tokens tokens
    finished = torch.zeros(B, dtype=torch.bool)
    exempt = 0
    for t in range(T):
        if t >= 1:
            for b in range(B):
                if finished[b]:
                    assert int(out[b, t]) == pad, (b, t)
                elif tie[b, t]:
                    exempt += 1
                else:
                    assert int(out[b, t]) == int(want[b, t]), (b, t, int(out[b, t]), int(want[b, t]), int(raw_am[b, t]))
        finished |= is_eos[:, t]
    assert exempt <= 1
    changed = (want != raw_am) & (want >= 0)
    assert bool(changed.any(1).all()), "the controls change no arg-max on this fixture: the comparison shows nothing"
    return want


PATHS = {"fused": {}, "unfused": {"decode_impl": "unfused"}, "op by op": {"native_step": False},
         "full scan": {"env": ("BRA_SAMPLE_TILES", "0")}, "shared prefix": {"copies": 2}, "per-copy decode": {"copies": 2, "shared_prefix_decode": False}}


@pytest.mark.parametrize("path", list(PATHS))
def test_teacher_forced_choices_follow_the_hf_processors(backend, monkeypatch, path):
    fix, m, b = _tiny_b(backend)
    opt = dict(PATHS[path])
    if "env" in opt:
        monkeypatch.setenv(*opt.pop("env"))
    copies = opt.pop("copies", 1)
    rows = [r for r in range(3) for _ in range(copies)]
    alias = [(j // copies) * copies for j in range(len(rows))] if copies > 1 else None
    T = fix["config"]["gen_tokens"]
    force = fix["fp32_lora"]["greedy_ids"][rows]
    eos = _eos_for(fix)
    tr = []
    out = m.generate(**_inputs(b, rows, alias), max_new_tokens=T, do_sample=False, eos_token_id=eos, pad_token_id=1, use_graph=False,
                     force_tokens=force.to(backend), trace_logits=tr, repetition_penalty=PEN, min_new_tokens=MIN_NEW, **opt)
    _check_forced(out, tr, force, eos, PEN, MIN_NEW, 1)


def _free_kw(fix, **over):
    kw = dict(max_new_tokens=8, do_sample=False, eos_token_id=_eos_for(fix), pad_token_id=1, use_graph=False, return_full_length=True,
              repetition_penalty=PEN, min_new_tokens=MIN_NEW)
    kw.update(over)
    return kw


def test_free_running_paths_agree_with_the_controls_on(backend, monkeypatch):
    fix, m, b = _tiny_b(backend)
    rows = [0, 1, 2]
    plain = m.generate(**_inputs(b, rows), **_free_kw(fix, repetition_penalty=1.0, min_new_tokens=0))
    tiles = m.generate(**_inputs(b, rows), **_free_kw(fix))
    assert tiles.shape == (3, 8) and not torch.equal(tiles, plain)
    for e in _eos_for(fix):
        assert not bool((tiles[:, :MIN_NEW] == e).any())
    monkeypatch.setenv("BRA_SAMPLE_TILES", "0")
    scan = m.generate(**_inputs(b, rows), **_free_kw(fix))
    monkeypatch.delenv("BRA_SAMPLE_TILES")
    assert torch.equal(tiles, scan)                                          # tile-maxima sampler == full-scan sampler
    # sampling with min_p: one seed, one rollout; and the filter is in force (min_p = 1 keeps the top token only: greedy)
    skw = _free_kw(fix, do_sample=True, temperature=20.0, top_k=20, top_p=0.95, min_p=0.2, seed=5)
    s1, s2 = m.generate(**_inputs(b, rows), **skw), m.generate(**_inputs(b, rows), **skw)
    assert torch.equal(s1, s2)
    assert torch.equal(m.generate(**_inputs(b, rows), **dict(skw, min_p=1.0)), tiles)
    assert not torch.equal(m.generate(**_inputs(b, rows), **dict(skw, min_p=None)), tiles)


def test_row_chunks_carry_the_controls(backend, monkeypatch):
    """20 rows through the default 16-row chunks == the same rows decoded as two calls"""
    fix, m, b = _tiny_b(backend)
    rows20 = [0] * 7 + [1] * 7 + [2] * 6
    seen = []
    real = generation._generate_in_row_chunks
    monkeypatch.setattr(generation, "_generate_in_row_chunks", lambda *a, **k: seen.append(1) or real(*a, **k))
    whole = m.generate(**_inputs(b, rows20), **_free_kw(fix))
    assert seen == [1]
    two = torch.cat([m.generate(**_inputs(b, rows20[:16]), **_free_kw(fix)), m.generate(**_inputs(b, rows20[16:]), **_free_kw(fix))], 0)
    assert len(seen) == 1 and whole.shape == (20, 8) and torch.equal(whole, two)
    plain = m.generate(**_inputs(b, rows20), **_free_kw(fix, repetition_penalty=1.0, min_new_tokens=0))
    assert not torch.equal(whole, plain)


@pytest.mark.gpu
def test_graph_replay_draws_what_eager_issue_draws(hip_device):
    """the processor launch is captured with the device-side step word: replay draws what eager issue draws (greedy and sampled,
    per-sequence and shared-prefix decode)"""
    backend = hip_device
    fix, m, b = _tiny_b(backend)
    for rows, alias in (([0, 1, 2], None), ([0, 0, 1, 1, 2, 2], [0, 0, 2, 2, 4, 4])):
        for over in ({}, dict(do_sample=True, temperature=20.0, top_k=20, top_p=0.95, min_p=0.2, seed=5)):
            kw = _free_kw(fix, max_new_tokens=24, **over)
            e = m.generate(**_inputs(b, rows, alias), **dict(kw, use_graph=False))
            g = m.generate(**_inputs(b, rows, alias), **dict(kw, use_graph=True))
            assert e.shape == g.shape == (len(rows), 24) and torch.equal(e, g)


def test_min_new_tokens_overrides_a_scheduled_eos(backend):
    """eos_schedule stands for the model's own logits, so min_new_tokens bans an EOS it schedules too early"""
    fix, m, b = _tiny_b(backend)
    eos, T = fix["config"]["eos_token_id"], 12
    kw = dict(max_new_tokens=T, do_sample=False, eos_token_id=eos, pad_token_id=1, use_graph=False, return_full_length=True,
              min_new_tokens=6)
    far = 1000
    early = m.generate(**_inputs(b, [0, 1, 2]), eos_schedule=torch.tensor([2, far, far], dtype=torch.int32, device=backend), **kw)
    assert early.shape == (3, T) and not bool((early[:, :6] == eos).any())
    unsched = m.generate(**_inputs(b, [0, 1, 2]), eos_schedule=torch.tensor([far] * 3, dtype=torch.int32, device=backend), **kw)
    # the banned EOS leaves the model's own choice: row 0 is not finished at step 2 (or 6) and decodes what it decodes unscheduled
    assert torch.equal(early, unsched) and not bool((early[0] == eos).any())
    late = m.generate(**_inputs(b, [0, 1, 2]), eos_schedule=torch.tensor([8, far, far], dtype=torch.int32, device=backend), **kw)
    assert int(late[0, 8]) == eos and bool((late[0, 9:] == 1).all()) and not bool((late[0, :8] == eos).any())
    assert torch.equal(late[1:], unsched[1:])
    off = m.generate(**_inputs(b, [0, 1, 2]), eos_schedule=torch.tensor([2, far, far], dtype=torch.int32, device=backend),
                     **dict(kw, min_new_tokens=0))
    assert int(off[0, 2]) == eos and bool((off[0, 3:] == 1).all())          # (without the control the schedule is honoured)


# ------------------------------------------------------------------------------------------------------- 5. public interface
def test_dna_llm_generate_honours_the_keywords(backend, monkeypatch):
    fix, m, b = _tiny_b(backend)
    T = fix["config"]["gen_tokens"]
    force = fix["fp32_lora"]["greedy_ids"]
    eos = _eos_for(fix)
    base = dict(max_new_tokens=T, do_sample=False, eos_token_id=eos, pad_token_id=1, use_graph=False, force_tokens=force.to(backend))
    tr = []
    out = m.generate(**_inputs(b, [0, 1, 2]), trace_logits=tr, repetition_penalty=PEN, min_new_tokens=MIN_NEW, min_p=0.5, **base)
    # fails on a build that drops the keywords: the output is then the raw arg-max, which _check_forced asserts differs
    _check_forced(out, tr, force, eos, PEN, MIN_NEW, 1)
    gc = SimpleNamespace(repetition_penalty=PEN, min_new_tokens=MIN_NEW, min_p=0.5, do_sample=False)
    via_gc = m.generate(**_inputs(b, [0, 1, 2]), generation_config=gc, **base)
    assert torch.equal(via_gc, out)
    weaker = m.generate(**_inputs(b, [0, 1, 2]), generation_config=gc, repetition_penalty=1.0, **base)       # a keyword wins over the config
    assert not torch.equal(weaker, out)
    # defaults: the tokens of a call without the keywords, and not one launch of the processor
    calls = []
    real = ops.logits_process
    monkeypatch.setattr(ops, "logits_process", lambda *a, **k: calls.append(1) or real(*a, **k))
    plain = m.generate(**_inputs(b, [0, 1, 2]), **base)
    dflt = m.generate(**_inputs(b, [0, 1, 2]), repetition_penalty=1.0, min_new_tokens=0, min_p=None, **base)
    assert torch.equal(plain, dflt) and calls == []
    skw = dict(max_new_tokens=T, do_sample=True, temperature=0.8, top_k=20, top_p=0.95, seed=3, eos_token_id=None, use_graph=False)
    assert torch.equal(m.generate(**_inputs(b, [0, 1, 2]), **skw),
                       m.generate(**_inputs(b, [0, 1, 2]), repetition_penalty=1.0, min_new_tokens=0, min_p=None, **skw))
    assert calls == []
    m.generate(**_inputs(b, [0, 1, 2]), min_new_tokens=2, **base)
    assert len(calls) == T
    for bad in (dict(repetition_penalty=0), dict(repetition_penalty=-1.0), dict(min_p=1.5), dict(min_p=-0.1, do_sample=True),
                dict(min_new_tokens=-1), dict(repetition_penalty=1.2, max_new_tokens=8193)):
        with pytest.raises(ValueError):
            m.generate(**_inputs(b, [0, 1, 2]), **dict(dict(max_new_tokens=T, do_sample=False, eos_token_id=None), **bad))


def test_grpo_config_carries_the_rollout_controls(backend):
    from test_model_parity import build
    from test_shared_policy import _group_batch
    from bioreason_amd.trainer import GRPOConfig, GRPOStepRunner
    fix = torch.load(os.path.join(GOLD, "tiny_b.pt"), weights_only=False)
    common = dict(num_generations=2, max_completion_length=6, eos_token_id=None, seed=3, learning_rate=1e-3, temperature=20.0)
    # (temperature 20: the fixture's top logit leads by ~30, so a usual temperature draws one token whatever the controls do)

    def one_step(**over):
        m = build(fix, backend, True)
        ids, mask, mm, alias = _group_batch(fix, backend, 2)
        batch = {"input_ids": ids, "attention_mask": mask, "dna_tokenized": mm["dna_tokenized"], "batch_idx_map": mm["batch_idx_map"],
                 "prompt_alias": alias}
        cfg = GRPOConfig(**common, **over)
        direct = m.generate(input_ids=ids, attention_mask=mask, **mm, dna_alias=None, max_new_tokens=cfg.max_completion_length,
                            do_sample=True, temperature=cfg.temperature, top_k=cfg.top_k, top_p=cfg.top_p, eos_token_id=None,
                            pad_token_id=None, seed=cfg.seed, return_full_length=True, prompt_alias=alias, use_graph=cfg.rollout_graph,
                            shared_prefix_decode=cfg.rollout_shared_prefix)
        runner = GRPOStepRunner(m, cfg)
        out = runner.step(batch)
        assert torch.isfinite(out["loss_t"]).all()
        return runner._buffered_inputs[0]["completion_ids"], direct

    assert GRPOConfig().repetition_penalty == 1.0 and GRPOConfig().min_p is None
    dflt, direct = one_step()
    assert torch.equal(dflt, direct)                     # the default config rolls out what a call without the controls rolls out
    ctl, _ = one_step(repetition_penalty=1.2, min_p=0.05)
    assert ctl.shape == dflt.shape and not torch.equal(ctl, dflt)
