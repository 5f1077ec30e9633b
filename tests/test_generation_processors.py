"""sequence_bias, no_repeat_ngram_size, bad_words_ids, suppress_tokens and begin_suppress_tokens in the token loop
(bra_logits_process_ext: the whole processor chain in one launch in front of the samplers).

The yardstick is the installed `transformers.generation.logits_process` classes on the CPU in fp32, in the order of
GenerationMixin._get_logits_processor: SequenceBias -> RepetitionPenalty -> NoRepeatNGram -> NoBadWords -> MinNewTokensLength ->
SuppressTokens -> SuppressTokensAtBegin, over the GENERATED tokens only and with begin_index = 0 —
`test_hf_applies_the_chain_to_generated_tokens_only` pins that this is what HF does for generate(inputs_embeds=...)."""
import os
from types import SimpleNamespace

import pytest
import torch
from transformers.generation.logits_process import (MinNewTokensLengthLogitsProcessor, NoBadWordsLogitsProcessor,
                                                    NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor,
                                                    SequenceBiasLogitsProcessor, SuppressTokensAtBeginLogitsProcessor,
                                                    SuppressTokensLogitsProcessor)

from bioreason_amd import generation, ops
from bioreason_amd._lib import KernelError
from test_generation_controls import PATHS, _inputs, _tiny_b, ulp_dist

GOLD = os.path.join(os.path.dirname(__file__), "golden")
SENT = -77.0
NINF = float("-inf")


def hf_chain(scores, hist, pen=1.0, mn=0, eos_ids=(), ngram=0, seq_bias=None, bad_words=None, sup=None, bsup=None):
    """the installed HF processors in HF's order on CPU scores [B, V] with the generated-only history `hist` [B, t] (long).
    `bad_words` as the caller gives them (HF drops the [eos] words itself)."""
    out = scores.clone()
    eos_ids = [e for e in eos_ids if e >= 0]
    if seq_bias:
        out = SequenceBiasLogitsProcessor(dict(seq_bias))(hist, out)
    if pen != 1.0 and hist.shape[1] > 0:
        out = RepetitionPenaltyLogitsProcessor(float(pen))(hist, out)
    if ngram:
        out = NoRepeatNGramLogitsProcessor(int(ngram))(hist, out)
    if bad_words:
        drop = [w for w in bad_words if not (len(w) == 1 and w[0] in eos_ids)]
        if drop:
            out = NoBadWordsLogitsProcessor([list(w) for w in bad_words], eos_ids or None)(hist, out)
    if mn > 0 and eos_ids:
        out = MinNewTokensLengthLogitsProcessor(0, int(mn), eos_ids, device="cpu")(hist, out.clone())
    if sup:
        out = SuppressTokensLogitsProcessor(list(sup))(hist, out)
    if bsup:
        out = SuppressTokensAtBeginLogitsProcessor(list(bsup), 0)(hist, out)
    return out


def bits(x):
    return x.contiguous().view(torch.int32)


# ----------------------------------------------------------------------------------------------------- 1. semantics pin (CPU)
def test_hf_applies_the_chain_to_generated_tokens_only():
    """HF generate(inputs_embeds=..., the five keywords) == a plain loop applying the chain to the generated-only history with
    begin_index 0, and != the call without the keywords (float64: no near-ties between cached and uncached forwards)"""
    from oracle.dna_llm_oracle import make_qwen3
    torch.manual_seed(2)
    V, P, T, B = 64, 16, 12, 2
    hf = make_qwen3({"vocab_size": V, "hidden_size": 32, "intermediate_size": 64, "num_hidden_layers": 2, "num_attention_heads": 2,
                     "num_key_value_heads": 1, "head_dim": 16}).double().eval()
    prompt = torch.stack([torch.randperm(V) for _ in range(B)])[:, :P]
    emb = hf.get_input_embeddings()
    mask = torch.ones(B, P, dtype=torch.long)

    def logits_after(gen):
        ids = torch.cat([prompt, gen], 1)
        with torch.no_grad():
            return hf(inputs_embeds=emb(ids), attention_mask=torch.ones_like(ids)).logits[:, -1]

    def loop(ctl):
        gen = torch.zeros(B, 0, dtype=torch.long)
        for _ in range(T):
            sc = hf_chain(logits_after(gen), gen, **ctl)
            gen = torch.cat([gen, sc.argmax(-1)[:, None]], 1)
        return gen

    plain = loop({})
    # controls taken from what the model does unhindered, so that each of them bites: the first token of row 0 is suppressed at the
    # beginning, row 1's second token always, row 0's third bigram is a bad word, and a bias lifts a token the rows never chose
    spare = [v for v in range(1, V) if v not in plain.tolist()[0] + plain.tolist()[1]]
    ctl = dict(ngram=2, bsup=[int(plain[0, 0])], sup=[int(plain[1, 1])], bad_words=[[int(plain[0, 2]), int(plain[0, 3])]],
               seq_bias={(spare[0],): 1.5, (int(plain[1, 0]), spare[1]): 4.0})
    with torch.no_grad():
        out = hf.generate(inputs_embeds=emb(prompt), attention_mask=mask, max_new_tokens=T, do_sample=False, eos_token_id=None,
                          pad_token_id=0, no_repeat_ngram_size=2, bad_words_ids=ctl["bad_words"], suppress_tokens=ctl["sup"],
                          begin_suppress_tokens=ctl["bsup"], sequence_bias=ctl["seq_bias"])
        base = hf.generate(inputs_embeds=emb(prompt), attention_mask=mask, max_new_tokens=T, do_sample=False, eos_token_id=None,
                           pad_token_id=0)
    own = loop(ctl)
    assert torch.equal(base, plain)
    assert out.shape == own.shape and torch.equal(out, own)
    assert not torch.equal(out, base) and bool((out != base).any(1).all())
    assert int(out[0, 0]) != int(plain[0, 0]) and not bool((out == int(plain[1, 1])).any())


# --------------------------------------------------------------------------------- 2. ops.logits_process_ext vs the HF processors
LP_B, LP_V = 3, 5000                       # >= 4096, not a multiple of 16 (ragged last tile: columns 4992 .. 4999)
LP_EOS = (4990, 17)
S_TOK, S2_TOK, MAXTILE_TOK, LIFT_TOK, FLIP_TOK, NINF_TOK, BAD2_TOK = 1000, 1100, 2000, 3000, 7, 3500, 2600
B0, B1, B2 = 1.1, 0.7, 0.3                 # fp32: (B0 + B1) + B2 != (B0 + B2) + B1 (asserted below)
LP_SUP = [4990, 40, LP_V, LP_V + 77, -3]   # an EOS id, a plain id, ids past the vocabulary and a negative one
LP_BSUP = [5, 4996, LP_V + 1]              # one of the ragged tile
LP_TS = {n: sorted({0, 1, n - 1, n, 5, 300}) for n in (1, 2, 3, 4)}


def _lp_inputs():
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(LP_B, LP_V, generator=g) * 3.0
    assert not bool((logits == 0).any())
    logits[:, 7], logits[:, 8], logits[:, 0], logits[:, 4995] = 2.5, -1.25, -0.3, 14.0
    logits[1, 7], logits[2, 4995] = -2.5, -0.75
    logits[:, MAXTILE_TOK] = 15.0                                         # the maximum of its tile (a bad word removes it)
    logits[:, LIFT_TOK] = -9.0                                            # far below its tile's maximum (a bias of +50 makes it that)
    hist = torch.empty(LP_B, 320, dtype=torch.long)
    # row 0: four equal tokens (id 0: at t = n the only window bans id 0), then a period of five with the last column of the
    # vocabulary and a column of the ragged tile; row 1: a period of seven with a doubled id; row 2: 40 ids at random
    p0, p1 = torch.tensor([11, 4999, 12, 4995, 13]), torch.tensor([7, 7, 8, 0, 4999, 2500, 4995])
    hist[0] = torch.cat([torch.zeros(4, dtype=torch.long), p0.repeat(64)])[:320]
    hist[1] = p1.repeat(46)[:320]
    pool = torch.randint(0, LP_V, (40,), generator=g)
    hist[2] = pool[torch.randint(0, 40, (320,), generator=g)]
    hist[2, :5] = torch.tensor([7, 7, 8, 0, 4995])
    return logits, hist


def _lp_tables(hist, t):
    """the sequence tables of step t -> (sequence_bias dict in HF's form, bad words).  The multi-token sequences are cut from the
    tail of row 0's (row 1's) history so that they match there at this t; a multi-token key stands BEFORE the single-token key of
    the same last token in the dict (HF still adds the single-token bias first)."""
    h0, h1 = hist[0].tolist(), hist[1].tolist()
    sb = {}
    if t >= 2:
        sb[(h0[t - 1], S_TOK)] = B1                                       # two longer sequences ending in the single-token bias's token
    if t >= 3:
        sb[(h0[t - 2], h0[t - 1], S_TOK)] = B2
    sb[(S_TOK,)] = B0
    sb[(LIFT_TOK,)] = 50.0                                                # makes its token the new maximum of its tile
    sb[(FLIP_TOK,)] = -4.0                                                # rows 0, 2: l = 2.5 > 0 > l + b, and 7 is in the history
    sb[(NINF_TOK,)] = NINF
    if t >= 1:
        sb[(h0[t - 1], S2_TOK)] = NINF                                    # -inf and a finite bias in one group
        sb[(S2_TOK,)] = 1.0
        sb[tuple(h0[1:t]) + (LIFT_TOK + 1,)] = 3.0                        # L = t exactly: acts (t = 1: a single token)
        sb[tuple(h0[:t]) + (LIFT_TOK + 2,)] = 3.0                         # L = t + 1: its prefix IS the history, and it must not act
    bad = [[MAXTILE_TOK], [LP_EOS[0]]]                                    # ([eos] is dropped by HF and by the host when eos is set)
    if t >= 1:
        bad += [[h1[t - 1], BAD2_TOK], h1[:t] + [BAD2_TOK + 1]]           # L = 2 on row 1's tail; L = t + 1 must not act
    return sb, bad


def test_bias_constants_show_the_order_of_accumulation():
    f = lambda x: torch.tensor(x, dtype=torch.float32)
    assert not torch.equal((f(B0) + f(B1)) + f(B2), (f(B0) + f(B2)) + f(B1))


@pytest.mark.parametrize("step_kind", ["device_word", "int"])
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_logits_process_ext_matches_hf_processors(backend, n, step_kind):
    dev = backend
    logits, hist = _lp_inputs()
    hist_d = hist.to(torch.int32).to(dev)
    ngram_banned = torch.zeros(LP_V, dtype=torch.bool)
    for t in LP_TS[n]:
        step = torch.tensor([t], dtype=torch.int32, device=dev) if step_kind == "device_word" else t
        sb, bad = _lp_tables(hist, t)
        h = hist[:, :t]
        for pen, mn, eos in ((1.3, t + 1, LP_EOS), (0.8, 0, (-1, -1)), (1.0, t + 3, (LP_EOS[0], -1))):
            eos_l = [e for e in eos if e >= 0]
            bad_host = [w for w in bad if not (len(w) == 1 and w[0] in eos_l)]
            ctl = dict(pen=pen, mn=mn, eos_ids=eos, ngram=n, seq_bias=sb, bad_words=bad, sup=LP_SUP, bsup=LP_BSUP)
            want = hf_chain(logits, h, **ctl)
            biased = SequenceBiasLogitsProcessor(dict(sb))(h, logits.clone())           # the values the penalty sees
            tables = ops.ProcessorTables(LP_V, dev, ngram=n, sequence_bias=sb, bad_words=bad_host, suppress=LP_SUP,
                                         begin_suppress=LP_BSUP)
            assert tables.over_capacity() is None
            buf = torch.full((LP_B + 2, LP_V), SENT, dtype=torch.float32)
            buf[:LP_B] = logits
            buf = buf.to(dev)
            lg = buf[:LP_B]
            tbuf = torch.full((LP_B + 2, (LP_V + 15) // 16), SENT, dtype=torch.float32, device=dev)
            tm = tbuf[:LP_B]
            ops.tile_max(lg, tm)
            ops.logits_process_ext(lg, hist_d, step, tables, pen, mn, eos[0], eos[1], None, tm)
            got = lg.cpu()
            key = (n, t, pen, mn, eos)
            banned = want == NINF
            assert bool((got[banned] == NINF).all()) and torch.equal(got == NINF, banned), key          # -inf exactly where HF has it
            in_table = torch.zeros(LP_B, LP_V, dtype=torch.bool)
            in_table[:, [k[-1] for k in sb]] = True
            seen = torch.zeros(LP_B, LP_V, dtype=torch.bool)
            if pen != 1.0 and t > 0:
                seen.scatter_(1, h, True)
            same = ~in_table & ~seen & ~banned
            assert torch.equal(bits(got[same]), bits(logits[same])), key                                  # untouched: bit-equal
            only_bias = in_table & ~seen & ~banned
            assert torch.equal(bits(got[only_bias]), bits(want[only_bias])), key                          # l + bias: bit-equal
            mul = seen & ~banned & (biased < 0)
            assert torch.equal(bits(got[mul]), bits(want[mul])), key                                      # l * penalty: bit-equal
            div = seen & ~banned & ~(biased < 0)
            assert int(ulp_dist(got[div], want[div]).max()) <= 2 if bool(div.any()) else True, key        # l / penalty: 2 ulp
            assert torch.equal(bits(tm.cpu()), bits(ops.tile_max(lg).cpu())), key                         # maxima of what is stored
            assert bool((buf[LP_B:] == SENT).all()) and bool((tbuf[LP_B:] == SENT).all()), key            # rows past B
            # the vectors do what they are there for
            assert float(want[0, S_TOK]) != float(logits[0, S_TOK]) and bool(banned[:, MAXTILE_TOK].all()) and bool(banned[:, NINF_TOK].all())
            assert not bool(banned[:, LIFT_TOK].any()) and float(tm[0, LIFT_TOK >> 4]) == float(want[0, LIFT_TOK])
            assert float(want[0, LIFT_TOK + 2]) == float(logits[0, LIFT_TOK + 2]), key                    # L = t + 1 does not act
            if t >= 1:
                assert float(want[0, LIFT_TOK + 1]) == float(logits[0, LIFT_TOK + 1] + 3.0), key          # L = t acts
                # two tokens act from t = 2 on, NOT at t = 1, and only where the tail of the row's history is their prefix
                assert bool(banned[0, S2_TOK]) == (t >= 2) and bool(banned[1, BAD2_TOK]) == (t >= 2), key
                assert bool(banned[1, S2_TOK]) == (t >= 2 and int(hist[1, t - 1]) == int(hist[0, t - 1])), key
                assert not bool(banned[:, BAD2_TOK + 1].any()), key
            if t >= 3:
                assert float(want[0, S_TOK]) == float((logits[0, S_TOK] + ((torch.tensor(B0) + B1) + B2))), key
            if pen != 1.0 and t >= 5:
                assert bool(mul[2, FLIP_TOK]) or n == 1, key                 # l > 0 > l + b: multiplied (n = 1 bans the token instead)
                assert float(logits[2, FLIP_TOK]) > 0 > float(biased[2, FLIP_TOK])
            assert bool(banned[:, LP_SUP[0]].all()) and bool(banned[:, 40].all()), key                    # suppressed, EOS or not
            assert bool(banned[:, 5].all()) == (t == 0) and bool(banned[:, 4996].all()) == (t == 0), key
            only_ngram = banned & ~(hf_chain(logits, h, **dict(ctl, ngram=0)) == NINF)
            ngram_banned |= only_ngram.any(0)
            if t < n:
                assert not bool(only_ngram.any()), key
    # over the steps of this n the n-gram ban has hit id 0, the last column and a column of the ragged tile
    assert bool(ngram_banned[0]) and bool(ngram_banned[LP_V - 1]) and bool(ngram_banned[4992:4999].any()), n
    # a finished row is left alone; the others are processed
    lg = logits.clone().to(dev)
    fin = torch.tensor([0, 1, 0], dtype=torch.uint8, device=dev)
    ops.logits_process_ext(lg, hist_d, step, tables, 1.3, t + 1, LP_EOS[0], -1, fin, None)
    assert torch.equal(lg[1].cpu(), logits[1]) and bool((lg[0].cpu() != logits[0]).any()) and bool((lg[2].cpu() != logits[2]).any())


@pytest.mark.parametrize("t", [0, 5, 300])
def test_old_controls_alone_leave_what_logits_process_leaves(backend, t):
    dev = backend
    logits, hist = _lp_inputs()
    hist_d = hist.to(torch.int32).to(dev)
    empty = ops.ProcessorTables(LP_V, dev)
    assert not empty.on
    for step in (t, torch.tensor([t], dtype=torch.int32, device=dev)):
        for pen, mn, eos in ((1.3, t + 1, LP_EOS), (0.8, 0, (-1, -1)), (1.0, t + 1, LP_EOS), (1.0, 0, LP_EOS)):
            a, b = logits.clone().to(dev), logits.clone().to(dev)
            ta, tb = ops.tile_max(a), ops.tile_max(b)
            ops.logits_process(a, hist_d, step, pen, mn, eos[0], eos[1], None, ta)
            ops.logits_process_ext(b, hist_d, step, empty, pen, mn, eos[0], eos[1], None, tb)
            assert torch.equal(bits(a.cpu()), bits(b.cpu())) and torch.equal(bits(ta.cpu()), bits(tb.cpu())), (t, pen, mn)


@pytest.mark.parametrize("t", [0, 5])
def test_lists_and_single_tokens_need_no_history(backend, t):
    """the two lists, single-token sequences and min_new_tokens read no history: none is handed in, and the step still counts (the
    begin list at t == 0 only, the EOS ban while t < min_new_tokens)"""
    dev = backend
    logits, hist = _lp_inputs()
    sb = {(S_TOK,): B0, (NINF_TOK,): NINF}
    tb = ops.ProcessorTables(LP_V, dev, sequence_bias=sb, bad_words=[[MAXTILE_TOK]], suppress=LP_SUP, begin_suppress=LP_BSUP)
    assert tb.on and not tb.multi_token
    for step in (t, torch.tensor([t], dtype=torch.int32, device=dev)):
        for mn in (t, t + 1):
            lg = logits.clone().to(dev)
            tm = ops.tile_max(lg)
            ops.logits_process_ext(lg, None, step, tb, 1.0, mn, LP_EOS[0], LP_EOS[1], None, tm)
            want = hf_chain(logits, hist[:, :t], mn=mn, eos_ids=LP_EOS, seq_bias=sb, bad_words=[[MAXTILE_TOK]], sup=LP_SUP, bsup=LP_BSUP)
            assert torch.equal(bits(lg.cpu()), bits(want)) and torch.equal(bits(tm.cpu()), bits(ops.tile_max(lg).cpu())), (t, mn)
            assert bool((want[:, 5] == NINF).all()) == (t == 0) and bool((want[:, LP_EOS[1]] == NINF).all()) == (t < mn)


def test_logits_process_ext_refuses_what_exceeds_its_limits(backend):
    """beyond a fixed limit: BRA_ERR_UNSUPPORTED and nothing written; at the limit: served; argument errors are argument errors"""
    dev = backend
    logits, hist = _lp_inputs()
    lg = logits.clone().to(dev)
    tm = ops.tile_max(lg)
    tm0 = tm.clone()
    T = ops.ProcessorTables
    wide = torch.zeros(LP_B, 8193, dtype=torch.int32)
    wide[:, :320] = hist
    wide = wide.to(dev)
    h_d = wide[:, :320].contiguous()
    over = [(h_d, 5, T(LP_V, dev, ngram=33)),
            (h_d, 5, T(LP_V, dev, bad_words=[[i + 1] for i in range(1025)])),
            (h_d, 5, T(LP_V, dev, sequence_bias={(i + 1,): 1.0 for i in range(1000)}, bad_words=[[i + 1] for i in range(25)])),
            (h_d, 5, T(LP_V, dev, bad_words=[list(range(1, 2050)), list(range(2, 2050))])),
            (h_d, 5, T(LP_V, dev, suppress=list(range(1025)))),
            (h_d, 5, T(LP_V, dev, begin_suppress=list(range(1025)))),
            (wide, 8193, T(LP_V, dev, ngram=2)),
            (wide, torch.tensor([3], dtype=torch.int32, device=dev), T(LP_V, dev, ngram=2))]
    for h, step, tb in over:
        assert tb.over_capacity() is not None or tb.ngram == 2
        with pytest.raises(KernelError) as ei:
            ops.logits_process_ext(lg, h, step, tb, 1.0, 0, -1, -1, None, tm)
        assert ei.value.status == -2
        assert torch.equal(lg.cpu(), logits) and torch.equal(tm, tm0)
    # at the limits: 1024 sequences of 4096 tokens, 1024 suppressed ids, n = 32 over 8192 entries
    bad = [[(7 * i) % (LP_V - 1) + 1] * 4 for i in range(1024)]
    tb = T(LP_V, dev, ngram=32, bad_words=bad, suppress=list(range(100, 1124)), begin_suppress=list(range(1200, 2224)))
    assert tb.over_capacity() is None and tb.n_tok == 4096
    h8 = wide[:, :8192].contiguous()
    ops.logits_process_ext(lg, h8, 8192, tb, 1.0, 0, -1, -1, None, tm)
    want = hf_chain(logits, h8.cpu().long(), ngram=32, bad_words=bad, sup=list(range(100, 1124)))
    assert torch.equal(bits(lg.cpu()), bits(want)) and torch.equal(tm, ops.tile_max(lg))
    assert bool((lg.cpu() == NINF)[:, 100:1124].all()) and not bool((lg.cpu() == NINF)[:, 1200:2224].all())
    sup = T(LP_V, dev, suppress=[3])
    with pytest.raises(KernelError) as ei:
        ops.logits_process_ext(lg, h_d, 5, sup, 0.0, 0, -1, -1, None, None)              # penalty must be > 0
    assert ei.value.status == -1
    with pytest.raises(KernelError) as ei:
        ops.logits_process_ext(lg, h_d[:, :4].contiguous(), 5, T(LP_V, dev, ngram=2), 1.0, 0, -1, -1, None, None)   # a step past the history
    assert ei.value.status == -1
    ops.logits_process_ext(lg, h_d[:, :4].contiguous(), 5, sup, 1.0, 0, -1, -1, None, None)      # (a list alone reads no history)
    with pytest.raises(KernelError) as ei:
        ops.logits_process_ext(lg, None, 5, T(LP_V, dev, ngram=2), 1.0, 0, -1, -1, None, None)    # an n-gram ban without a history
    assert ei.value.status == -1
    with pytest.raises(ValueError):
        T(LP_V, dev, bad_words=[[3, LP_V]])                                               # a sequence token past the vocabulary
    with pytest.raises(ValueError):
        T(LP_V, dev, sequence_bias={(LP_V + 3,): 1.0})
    ops.logits_process_ext(lg[:0], h_d[:0], 5, sup, 1.3, 0, -1, -1, None, None)          # B == 0


# ------------------------------------------------------------------------------------------- 3. end to end on the tiny_b fixture
def _plain_trace(m, b, rows, alias, force, T, backend, **opt):
    """teacher-forced, no controls: the raw logits of steps 1 .. T-1 (they do not depend on the controls: the forced token is fed back)"""
    tr = []
    out = m.generate(**_inputs(b, rows, alias), max_new_tokens=T, do_sample=False, eos_token_id=None, pad_token_id=1, use_graph=False,
                     force_tokens=force.to(backend), trace_logits=tr, **opt)
    return out.cpu(), [x.float().cpu() for x in tr]


def _controls_for(fix, V):
    """the fixture's greedy rows repeat one token each (245 / 214 / 291), so: the trigram ban bites from t = 3 on, the bad word
    [291, 291] bans row 2's token from t = 2 on (at t = 1 it must NOT: L - 1 tokens of history are not enough), the single-token bias
    moves row 1 at every step and the two-token bias row 0 from t = 2 on"""
    g = fix["fp32_lora"]["greedy_ids"]
    a, c, d = int(g[0, 0]), int(g[1, 0]), int(g[2, 0])
    return dict(no_repeat_ngram_size=3, bad_words_ids=[[d, d]], sequence_bias={(a, a): -1.0e4, (c,): -1.0e4},
                suppress_tokens=[V + 5, -2], begin_suppress_tokens=[a])


def _hf_kw(ctl, extra_sup=()):
    return dict(ngram=ctl["no_repeat_ngram_size"], seq_bias=ctl["sequence_bias"], bad_words=ctl["bad_words_ids"],
                sup=list(ctl["suppress_tokens"]) + list(extra_sup), bsup=ctl["begin_suppress_tokens"])


def _check_chain(out, trace, force, hfkw):
    """every token from t >= 1 on is the arg-max of the HF chain over the traced raw logits (HF top-2 within 4 ulp: exempt, at most
    one position); the controls change at least one arg-max in every row"""
    out = out.cpu()
    B, T = force.shape
    assert out.shape == (B, T) and len(trace) == T - 1
    exempt, changed = 0, torch.zeros(B, dtype=torch.bool)
    for t in range(1, T):
        raw = trace[t - 1]
        sc = hf_chain(raw, force[:, :t].long().cpu(), **hfkw)
        top2 = sc.topk(2, -1)[0]
        tie = ulp_dist(top2[:, 0], top2[:, 1]) <= 4
        want, raw_am = sc.argmax(-1), raw.argmax(-1)
        changed |= want != raw_am
        for r in range(B):
            if bool(tie[r]):
                exempt += 1
            else:
                assert int(out[r, t]) == int(want[r]), (r, t, int(out[r, t]), int(want[r]), int(raw_am[r]))
    assert exempt <= 1
    assert bool(changed.all()), "the controls change no arg-max in some row: the comparison shows nothing"
    return exempt


@pytest.mark.parametrize("path", list(PATHS))
def test_teacher_forced_choices_follow_the_hf_chain(backend, monkeypatch, path):
    fix, m, b = _tiny_b(backend)
    V = fix["config"]["text"]["vocab_size"]
    opt = dict(PATHS[path])
    if "env" in opt:
        monkeypatch.setenv(*opt.pop("env"))
    copies = opt.pop("copies", 1)
    rows = [r for r in range(3) for _ in range(copies)]
    alias = [(j // copies) * copies for j in range(len(rows))] if copies > 1 else None
    T = fix["config"]["gen_tokens"]
    force = fix["fp32_lora"]["greedy_ids"][rows]
    ctl = _controls_for(fix, V)
    plain, raw = _plain_trace(m, b, rows, alias, force, T, backend, **opt)
    # one more control from the raw logits: row 1's runner-up at t = 2 (its top token carries the bias) is suppressed as well
    runner_up = int(raw[1][copies].topk(2)[1][1])
    ctl["suppress_tokens"] = ctl["suppress_tokens"] + [runner_up]
    tr = []
    out = m.generate(**_inputs(b, rows, alias), max_new_tokens=T, do_sample=False, eos_token_id=None, pad_token_id=1, use_graph=False,
                     force_tokens=force.to(backend), trace_logits=tr, **ctl, **opt)
    tr = [x.float().cpu() for x in tr]
    assert all(torch.equal(x, y) for x, y in zip(tr, raw))                   # teacher forcing: the raw logits are the same
    exempt = _check_chain(out, tr, force, _hf_kw(ctl))
    assert exempt == 0                                                       # (these controls leave HF no near-tie on this fixture)
    assert not bool((out.cpu() == runner_up).any())
    # step 0 (the prefill's logits are not traced): the begin list moves row 0 off its first token and the single-token bias row 1;
    # nothing acts on row 2 yet
    first = out.cpu()[:, 0]
    assert not bool((first[:2 * copies] == plain[:2 * copies, 0]).any()) and torch.equal(first[2 * copies:], plain[2 * copies:, 0])


def test_teacher_forced_chain_with_penalty_and_min_new_tokens(backend):
    """the five controls together with the two earlier ones and EOS ids the rows reach for"""
    fix, m, b = _tiny_b(backend)
    V, T = fix["config"]["text"]["vocab_size"], fix["config"]["gen_tokens"]
    force = fix["fp32_lora"]["greedy_ids"]
    g = force
    eos = [int(g[0, 0]), int(g[1, 0])]
    ctl = _controls_for(fix, V)
    ctl["bad_words_ids"] = ctl["bad_words_ids"] + [[eos[0]]]                  # dropped: an [eos] word is no bad word
    base = dict(max_new_tokens=T, do_sample=False, eos_token_id=eos, pad_token_id=1, use_graph=False, force_tokens=force.to(backend),
                repetition_penalty=5.0, min_new_tokens=5)
    # what every row picks at t = 3 under the two earlier controls alone is suppressed as well: the five new controls then change
    # an arg-max in every row ON TOP of the earlier two (the guard below), so a build that drops them fails here
    old = m.generate(**_inputs(b, [0, 1, 2]), **base).cpu()
    ctl["suppress_tokens"] = ctl["suppress_tokens"] + sorted({int(x) for x in old[:, 3]} - set(eos))
    tr = []
    out = m.generate(**_inputs(b, [0, 1, 2]), trace_logits=tr, **base, **ctl).cpu()
    tr = [x.float().cpu() for x in tr]
    hfkw = dict(_hf_kw(ctl), pen=5.0, mn=5, eos_ids=eos)
    finished = torch.zeros(3, dtype=torch.bool)
    exempt, changed = 0, torch.zeros(3, dtype=torch.bool)
    for t in range(1, T):
        finished |= (out[:, t - 1] == eos[0]) | (out[:, t - 1] == eos[1])
        sc = hf_chain(tr[t - 1], force[:, :t].long(), **hfkw)
        changed |= ~finished & (sc.argmax(-1) != hf_chain(tr[t - 1], force[:, :t].long(), pen=5.0, mn=5, eos_ids=eos).argmax(-1))
        top2 = sc.topk(2, -1)[0]
        for r in range(3):
            if finished[r]:
                assert int(out[r, t]) == 1
            elif int(ulp_dist(top2[r, 0], top2[r, 1])) <= 4:
                exempt += 1
            else:
                assert int(out[r, t]) == int(sc[r].argmax()), (r, t)
    assert exempt <= 1
    assert bool(changed.all()), "the five controls change no arg-max on top of the earlier two in some row"
    assert not bool(((out[:, :5] == eos[0]) | (out[:, :5] == eos[1])).any())


def _free_kw(fix, V, **over):
    kw = dict(max_new_tokens=8, do_sample=False, eos_token_id=None, pad_token_id=1, use_graph=False, return_full_length=True,
              **_controls_for(fix, V))
    kw.update(over)
    return kw


OFF = dict(no_repeat_ngram_size=0, bad_words_ids=None, sequence_bias=None, suppress_tokens=None, begin_suppress_tokens=None)


def _assert_obeys(out, ctl):
    """free-running output: no trigram twice, no bad word of L tokens ending at a step >= L (HF lets it stand at the very
    beginning: with L - 1 tokens of history the sequence is still 'longer than the context'), no begin-suppressed first token"""
    for row in out.cpu().tolist():
        grams = [tuple(row[i:i + 3]) for i in range(len(row) - 2)]
        assert len(grams) == len(set(grams)), row
        for w in ctl["bad_words_ids"]:
            assert all(row[i:i + len(w)] != w for i in range(1, len(row) - len(w) + 1)), row
        assert row[0] not in ctl["begin_suppress_tokens"]


def test_free_running_paths_agree_with_the_processors_on(backend, monkeypatch):
    fix, m, b = _tiny_b(backend)
    V = fix["config"]["text"]["vocab_size"]
    rows = [0, 1, 2]
    plain = m.generate(**_inputs(b, rows), **_free_kw(fix, V, **OFF))
    tiles = m.generate(**_inputs(b, rows), **_free_kw(fix, V))
    assert tiles.shape == (3, 8) and bool((tiles != plain).any(1).all())
    _assert_obeys(tiles, _controls_for(fix, V))
    monkeypatch.setenv("BRA_SAMPLE_TILES", "0")
    scan = m.generate(**_inputs(b, rows), **_free_kw(fix, V))
    monkeypatch.delenv("BRA_SAMPLE_TILES")
    assert torch.equal(tiles, scan)                                          # tile-maxima sampler == full-scan sampler
    # one sampled rollout is reproducible under a seed, obeys the bans, and differs from the one without them
    skw = _free_kw(fix, V, do_sample=True, temperature=20.0, top_k=20, top_p=0.95, seed=5)
    s1, s2 = m.generate(**_inputs(b, rows), **skw), m.generate(**_inputs(b, rows), **skw)
    assert torch.equal(s1, s2)
    _assert_obeys(s1, _controls_for(fix, V))
    assert not torch.equal(s1, m.generate(**_inputs(b, rows), **dict(skw, seed=6)))


def test_row_chunks_carry_the_processors(backend, monkeypatch):
    """20 rows through the default 16-row chunks == the same rows decoded as two calls"""
    fix, m, b = _tiny_b(backend)
    V = fix["config"]["text"]["vocab_size"]
    rows20 = [0] * 7 + [1] * 7 + [2] * 6
    seen = []
    real = generation._generate_in_row_chunks
    monkeypatch.setattr(generation, "_generate_in_row_chunks", lambda *a, **k: seen.append(1) or real(*a, **k))
    monkeypatch.setenv("BRA_DEC_ROWS32", "0")
    whole = m.generate(**_inputs(b, rows20), **_free_kw(fix, V))
    assert seen == [1]
    two = torch.cat([m.generate(**_inputs(b, rows20[:16]), **_free_kw(fix, V)), m.generate(**_inputs(b, rows20[16:]), **_free_kw(fix, V))], 0)
    assert len(seen) == 1 and whole.shape == (20, 8) and torch.equal(whole, two)
    _assert_obeys(whole, _controls_for(fix, V))


def test_one_loop_of_32_rows_carries_the_processors(backend, monkeypatch):
    """BRA_DEC_ROWS32=1: 26 rows in ONE token loop draw what the 16-row loops draw.  (NOTES, "32 rows per weight stream": the 32-row
    projections are bit-identical to the 16-row kernels, which serve chunks of 9 .. 16 rows — so the chunks here are 16 + 10 rows,
    not 16 + a chunk of eight or fewer, whose 8-row kernels round differently.)"""
    fix, m, b = _tiny_b(backend)
    V = fix["config"]["text"]["vocab_size"]
    rows26 = [0] * 9 + [1] * 9 + [2] * 8
    seen = []
    real = generation._generate_in_row_chunks
    monkeypatch.setattr(generation, "_generate_in_row_chunks", lambda *a, **k: seen.append(1) or real(*a, **k))
    monkeypatch.setenv("BRA_DEC_ROWS32", "1")
    one = m.generate(**_inputs(b, rows26), **_free_kw(fix, V))
    assert seen == []
    monkeypatch.setenv("BRA_DEC_ROWS32", "0")
    chunks = m.generate(**_inputs(b, rows26), **_free_kw(fix, V))
    assert seen == [1] and one.shape == (26, 8) and torch.equal(one, chunks)
    _assert_obeys(one, _controls_for(fix, V))


@pytest.mark.gpu
def test_graph_replay_draws_what_eager_issue_draws_with_the_processors(hip_device):
    """the launch is captured with the device-side step word and nothing is carried between steps: replay == eager issue (greedy
    and sampled, per-sequence and shared-prefix decode)"""
    backend = hip_device
    fix, m, b = _tiny_b(backend)
    V = fix["config"]["text"]["vocab_size"]
    for rows, alias in (([0, 1, 2], None), ([0, 0, 1, 1, 2, 2], [0, 0, 2, 2, 4, 4])):
        for over in ({}, dict(do_sample=True, temperature=20.0, top_k=20, top_p=0.95, seed=5),
                     dict(OFF, suppress_tokens=[291, 208], begin_suppress_tokens=[245, 214], repetition_penalty=1.0)):   # no history kept
            kw = _free_kw(fix, V, max_new_tokens=24, **dict(dict(repetition_penalty=1.2), **over))
            e = m.generate(**_inputs(b, rows, alias), **dict(kw, use_graph=False))
            g = m.generate(**_inputs(b, rows, alias), **dict(kw, use_graph=True))
            assert e.shape == g.shape == (len(rows), 24) and torch.equal(e, g)
            if "suppress_tokens" in over:
                assert not bool(((g == 291) | (g == 208)).any()) and not bool(((g[:, 0] == 245) | (g[:, 0] == 214)).any())
            else:
                _assert_obeys(g, _controls_for(fix, V))


# ------------------------------------------------------------------------------------------------------- 4. public interface
def test_dna_llm_generate_honours_the_processor_keywords(backend, monkeypatch):
    fix, m, b = _tiny_b(backend)
    V, T = fix["config"]["text"]["vocab_size"], fix["config"]["gen_tokens"]
    force = fix["fp32_lora"]["greedy_ids"]
    ctl = _controls_for(fix, V)
    base = dict(max_new_tokens=T, do_sample=False, eos_token_id=None, pad_token_id=1, use_graph=False, force_tokens=force.to(backend))
    tr = []
    out = m.generate(**_inputs(b, [0, 1, 2]), trace_logits=tr, **ctl, **base)
    # fails on a build that drops the keywords: the output is then the raw arg-max, which _check_chain asserts differs in every row
    _check_chain(out, [x.float().cpu() for x in tr], force, _hf_kw(ctl))
    gc = SimpleNamespace(do_sample=False, **ctl)
    via_gc = m.generate(**_inputs(b, [0, 1, 2]), generation_config=gc, **base)
    assert torch.equal(via_gc, out)
    weaker = m.generate(**_inputs(b, [0, 1, 2]), generation_config=gc, no_repeat_ngram_size=0, sequence_bias={(3,): 0.5}, **base)
    assert not torch.equal(weaker, out)                                      # a keyword wins over the config
    # the list form of sequence_bias is the dict form
    as_list = m.generate(**_inputs(b, [0, 1, 2]), **dict(ctl, sequence_bias=[[list(k), v] for k, v in ctl["sequence_bias"].items()]), **base)
    assert torch.equal(as_list, out)
    # the lists alone (no history is kept for them): the begin list acts at step 0 and only there, the other at every step
    ref = m.generate(**_inputs(b, [0, 1, 2]), **base).cpu()
    only = m.generate(**_inputs(b, [0, 1, 2]), suppress_tokens=[int(ref[2, 3])], begin_suppress_tokens=[int(ref[1, 0])], **base).cpu()
    assert int(only[1, 0]) != int(ref[1, 0]) and torch.equal(only[:2, 1:], ref[:2, 1:]) and torch.equal(only[0], ref[0])
    assert int(ref[2, 3]) in ref[2].tolist() and int(ref[2, 3]) not in only[2].tolist()
    # defaults: the tokens of a call without the keywords, and not one launch of either processor entry point
    calls = []
    real, real_ext = ops.logits_process, ops.logits_process_ext
    monkeypatch.setattr(ops, "logits_process", lambda *a, **k: calls.append("old") or real(*a, **k))
    monkeypatch.setattr(ops, "logits_process_ext", lambda *a, **k: calls.append("ext") or real_ext(*a, **k))
    plain = m.generate(**_inputs(b, [0, 1, 2]), **base)
    dflt = m.generate(**_inputs(b, [0, 1, 2]), **OFF, **base)
    assert torch.equal(plain, dflt) and calls == []
    m.generate(**_inputs(b, [0, 1, 2]), min_new_tokens=2, **base)           # an old control alone: the old entry point alone
    assert calls == ["old"] * T
    del calls[:]
    m.generate(**_inputs(b, [0, 1, 2]), min_new_tokens=2, suppress_tokens=[3], **base)     # a new one on: the new entry point alone
    assert calls == ["ext"] * T
    bad_values = (dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=2.0), dict(no_repeat_ngram_size=33),
                  dict(no_repeat_ngram_size=2, max_new_tokens=8193),
                  dict(bad_words_ids=[]), dict(bad_words_ids=[3, 4]), dict(bad_words_ids=[[3, -1]]), dict(bad_words_ids=[[3.0]]),
                  dict(bad_words_ids=[[3, V]]), dict(bad_words_ids=[[i + 1] for i in range(1025)]),
                  dict(sequence_bias={}), dict(sequence_bias={3: 1.0}), dict(sequence_bias={(3,): 1}), dict(sequence_bias={(-3,): 1.0}),
                  dict(sequence_bias={(3,): float("inf")}), dict(sequence_bias={(3,): float("nan")}), dict(sequence_bias={(V,): 1.0}),
                  dict(sequence_bias=[[[3], 1]]), dict(sequence_bias=[[3, 1.0]]),
                  dict(suppress_tokens=[1.5]), dict(suppress_tokens="12"), dict(begin_suppress_tokens=[None]),
                  dict(suppress_tokens=list(range(1025))))
    for bad in bad_values:
        with pytest.raises(ValueError):
            m.generate(**_inputs(b, [0, 1, 2]), **dict(dict(max_new_tokens=T, do_sample=False, eos_token_id=None), **bad))
    assert calls == ["ext"] * T                                              # (every refusal came before any launch)
    ok = m.generate(**_inputs(b, [0, 1, 2]), sequence_bias={(3,): float("-inf")}, suppress_tokens=[V + 9, -4], **base)
    assert torch.equal(ok, plain)                                            # -inf is a bias; ids outside the vocabulary do nothing


def test_grpo_config_carries_the_processors(backend):
    from test_model_parity import build
    from test_shared_policy import _group_batch
    from bioreason_amd.trainer import GRPOConfig, GRPOStepRunner
    fix = torch.load(os.path.join(GOLD, "tiny_b.pt"), weights_only=False)
    common = dict(num_generations=2, max_completion_length=6, eos_token_id=None, seed=3, learning_rate=1e-3, temperature=20.0)

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

    c0 = GRPOConfig()
    assert c0.no_repeat_ngram_size == 0 and c0.bad_words_ids is None and c0.suppress_tokens is None
    dflt, direct = one_step()
    assert torch.equal(dflt, direct)                     # the default config rolls out what a call without the controls rolls out
    seen = sorted(set(dflt.cpu().flatten().tolist()))
    ctl, _ = one_step(no_repeat_ngram_size=1, bad_words_ids=[[seen[0]]], suppress_tokens=[seen[-1]])
    assert ctl.shape == dflt.shape and not torch.equal(ctl, dflt)
    assert seen[0] not in ctl.cpu().flatten().tolist() and seen[-1] not in ctl.cpu().flatten().tolist()
    for row in ctl.cpu().tolist():
        assert len(set(row)) == len(row)                 # n = 1: no token twice
