"""generate(return_logprobs=True) and the GRPO step with rollout_is_correction: the token loop reports, per recorded token, the
log-probability its own network gave it (raw logits, temperature 1, whole vocabulary), on every path of the loop, and the step
runner hands it to the truncated-importance-sampling loss.

The tiny model of the generation-control tests (tests/golden/tiny_b.pt), 12 new tokens, sampling with the GRPO warpers (temperature
20: the fixture's top logit leads by ~30, so a usual temperature draws one token whatever else happens), one group of 4 copies plus a
second prompt — [0, 0, 0, 0, 1] for the per-sequence loop, [0] * 4 + [1] * 4 for the shared-prefix loop.

No test here asserts how close the rollout's and the trainer's log-probs are: the trainer tests print rollout_kl / is_mean / is_capped.
"""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bioreason_amd import generation, grpo, ops                        # noqa: E402
from bioreason_amd._lib import get_lib                                 # noqa: E402
from test_token_logp import U32, _depth                                # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")
F32, F64 = torch.float32, torch.float64
T = 12
SAMPLING = dict(do_sample=True, temperature=20.0, top_k=20, top_p=0.95, seed=5)
FAR = 1000


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


GROUP5 = ([0, 0, 0, 0, 1], [0, 0, 0, 0, 4])              # one group of 4 copies + a second prompt: the per-sequence loop
GROUP8 = ([0] * 4 + [1] * 4, [0] * 4 + [4] * 4)          # two groups of 4: the shared-prefix loop
PATHS = {"fused": (GROUP5, {}), "unfused": (GROUP5, {"decode_impl": "unfused"}), "op by op": (GROUP5, {"native_step": False}),
         "full scan": (GROUP5, {"env": ("BRA_SAMPLE_TILES", "0")}), "shared prefix": (GROUP8, {}),
         "per-copy decode": (GROUP8, {"shared_prefix_decode": False}), "no alias": (([0, 1, 2], None), {})}


def _kw(**over):
    kw = dict(max_new_tokens=T, eos_token_id=None, use_graph=False, return_full_length=True, return_logprobs=True, **SAMPLING)
    kw.update(over)
    return kw


def _check_against_trace(tok, lp, trace, first_step=1):
    """lp[:, t] (t >= 1) against the float64 log-softmax of the traced logits at the recorded token, within the kernel bound of
    tests/test_token_logp.py: E = ulp32(|x_tok|) + ulp32(|lse|) + D u, allowed ratio twice the fp32 twin's worst over the same logits"""
    tok, lp = tok.cpu(), lp.cpu()
    worst = twin_worst = 0.0
    for t in range(first_step, tok.shape[1]):
        x = trace[t - 1].float().cpu()
        V = x.shape[1]
        idx = tok[:, t].long()[:, None]
        x64 = x.to(F64)
        lse = torch.logsumexp(x64, 1)
        xt = x64.gather(1, idx)[:, 0]
        ref = xt - lse
        E = 2 * U32 * (xt.abs() + lse.abs()) + _depth(V) * U32
        m = x.max(1, keepdim=True).values
        twin = x.gather(1, idx)[:, 0] - (m[:, 0] + (x - m).exp().sum(1).log())
        worst = max(worst, ((lp[:, t].to(F64) - ref).abs() / E).max().item())
        twin_worst = max(twin_worst, ((twin.to(F64) - ref).abs() / E).max().item())
    print(f"\n[rollout-logp] vs trace: kernel {worst:.4f} twin {twin_worst:.4f}")
    assert worst <= 2 * twin_worst, (worst, twin_worst)


@pytest.mark.parametrize("path", list(PATHS))
def test_logprobs_are_the_log_softmax_of_the_traced_logits(backend, monkeypatch, path):
    fix, m, b = _tiny_b(backend)
    (rows, alias), opt = PATHS[path]
    opt = dict(opt)
    if "env" in opt:
        monkeypatch.setenv(*opt.pop("env"))
    tr = []
    tok, lp = m.generate(**_inputs(b, rows, alias), trace_logits=tr, **_kw(**opt))
    assert tok.shape == (len(rows), T) and lp.shape == tok.shape and lp.dtype == F32 and tok.dtype == torch.long
    assert len(tr) == T - 1
    assert bool(torch.isfinite(lp).all()) and bool((lp <= 0).all()) and bool((lp[:, 0] < 0).any())      # (0.0: a top token that leads by ~30)
    assert len(set(tok[:, 1:].reshape(-1).tolist())) > 4, "the draws are all one token: the comparison shows little"
    _check_against_trace(tok, lp, tr)
    # the flag off: a bare tensor, the same tokens for the same seed, and not one launch of the kernel
    calls = []
    real = ops.token_logp
    monkeypatch.setattr(ops, "token_logp", lambda *a, **k: calls.append(1) or real(*a, **k))
    off = m.generate(**_inputs(b, rows, alias), **_kw(return_logprobs=False, **opt))
    assert isinstance(off, torch.Tensor) and torch.equal(off, tok) and calls == []
    m.generate(**_inputs(b, rows, alias), **_kw(**opt))
    assert len(calls) == T


def test_logprobs_under_force_tokens_belong_to_the_recorded_token(backend):
    """teacher forcing feeds the given token back and records the model's own choice: the value is the recorded token's"""
    fix, m, b = _tiny_b(backend)
    rows, alias = GROUP5
    free, _ = m.generate(**_inputs(b, rows, alias), **_kw())
    force = free.flip(0).contiguous()                              # (other rows' tokens: the fed token differs from the recorded one)
    tr = []
    tok, lp = m.generate(**_inputs(b, rows, alias), force_tokens=force.to(backend), trace_logits=tr, **_kw())
    assert not torch.equal(tok, force)
    _check_against_trace(tok, lp, tr)


def test_sub_batch_reports_the_bits_of_the_whole_batch(backend):
    """the same rows as one loop and as a sub-batch — the leading rows of the batch, same seed, so the draws coincide: bit-identical"""
    fix, m, b = _tiny_b(backend)
    # (both prompts stay in the sub-batch: the prompt pass then runs the same two distinct prompts)
    tok5, lp5 = m.generate(**_inputs(b, [0, 0, 1, 1, 1], [0, 0, 2, 2, 2]), **_kw())
    tok3, lp3 = m.generate(**_inputs(b, [0, 0, 1], [0, 0, 2]), **_kw())
    assert torch.equal(tok3, tok5[:3])
    assert torch.equal(lp3.cpu().view(torch.int32), lp5[:3].cpu().view(torch.int32))


@pytest.mark.gpu
def test_graph_replay_reports_what_eager_issue_reports(hip_device):
    """the kernel is captured inside the replayed body and reads the device-side step word: same tokens, same bits"""
    fix, m, b = _tiny_b(hip_device)
    for rows, alias in (GROUP5, GROUP8, ([0, 1, 2], None)):
        for over in ({}, dict(eos_token_id=fix["config"]["eos_token_id"], pad_token_id=1,
                              eos_schedule=torch.tensor([3, FAR, 7, 20, 5, FAR, FAR, 2][:len(rows)], dtype=torch.int32, device=hip_device))):
            kw = _kw(max_new_tokens=24, **over)
            te, le = m.generate(**_inputs(b, rows, alias), **dict(kw, use_graph=False))
            tg, lg = m.generate(**_inputs(b, rows, alias), **dict(kw, use_graph=True))
            assert te.shape == tg.shape == (len(rows), 24) and torch.equal(te, tg)
            assert torch.equal(le.cpu().view(torch.int32), lg.cpu().view(torch.int32))
            assert bool((le[:, 1:] < 0).any())


def _zeros_after_eos(tok, lp, eos):
    tok, lp = tok.cpu(), lp.cpu()
    e = (tok == eos).int()
    after = (e.cumsum(1) - e) > 0
    assert bool((lp[after] == 0.0).all()), "a position after a row's first EOS is not exactly 0.0"
    return after


def test_zeros_after_eos_under_a_schedule(backend):
    """eos_schedule: the value is over the logits as the schedule left them (the scheduled EOS itself: log-probability 0.0, its logit
    1e30 above the rest); every position after the first EOS holds exactly 0.0; the trimming is the tokens'"""
    fix, m, b = _tiny_b(backend)
    eos = fix["config"]["eos_token_id"]
    rows, alias = GROUP8
    sched = torch.tensor([2, FAR, 5, 0, FAR, 9, 3, 11], dtype=torch.int32, device=backend)
    kw = _kw(eos_token_id=eos, pad_token_id=1, eos_schedule=sched)
    tok, lp = m.generate(**_inputs(b, rows, alias), **kw)
    assert tok.shape == lp.shape == (8, T)
    after = _zeros_after_eos(tok, lp, eos)
    live = ~after & (tok.cpu() != eos)
    assert bool(after.any()) and bool((lp.cpu()[live] <= 0).all()) and bool((lp.cpu()[live] < 0).any())
    for r, s in enumerate(sched.tolist()):
        if s < T:
            assert int(tok[r, s]) == eos and float(lp[r, s]) == 0.0 and bool((tok[r, s + 1:] == 1).all())
    # trimmed like the tokens: every row finished by step 6 -> 7 columns
    sched2 = torch.tensor([2, 6, 5, 0, 1, 4, 3, 2], dtype=torch.int32, device=backend)
    tok2, lp2 = m.generate(**_inputs(b, rows, alias), **dict(kw, eos_schedule=sched2, return_full_length=False))
    assert tok2.shape == lp2.shape == (8, 7)
    _zeros_after_eos(tok2, lp2, eos)
    bare = m.generate(**_inputs(b, rows, alias), **dict(kw, eos_schedule=sched2, return_full_length=False, return_logprobs=False))
    assert torch.equal(bare, tok2)


def test_twenty_rows_in_row_chunks_and_in_one_loop(backend, monkeypatch):
    """20 rows: the default 16-row chunks stitch the log-prob matrices back like the tokens (== the chunks as separate calls); with
    BRA_DEC_ROWS32=1, where the shapes have the 32-row forms, one loop: shapes and zeros after EOS"""
    fix, m, b = _tiny_b(backend)
    eos = fix["config"]["eos_token_id"]
    rows20 = [0] * 7 + [1] * 7 + [2] * 6
    alias20 = [0] * 7 + [7] * 7 + [14] * 6
    sched = torch.tensor([(3 * r) % 14 for r in range(20)], dtype=torch.int32, device=backend)       # (12, 13: never within T)
    kw = _kw(eos_token_id=eos, pad_token_id=1, eos_schedule=sched)
    seen = []
    real = generation._generate_in_row_chunks
    monkeypatch.setattr(generation, "_generate_in_row_chunks", lambda *a, **k: seen.append(1) or real(*a, **k))
    tok, lp = m.generate(**_inputs(b, rows20, alias20), **kw)
    assert seen == [1] and tok.shape == lp.shape == (20, T)
    _zeros_after_eos(tok, lp, eos)
    ta, la = m.generate(**_inputs(b, rows20[:14], alias20[:14]), **dict(kw, eos_schedule=sched[:14].contiguous()))
    tb, lb = m.generate(**_inputs(b, rows20[14:], [0] * 6), **dict(kw, eos_schedule=sched[14:].contiguous(), seed=SAMPLING["seed"] + 7919))
    assert len(seen) == 1
    assert torch.equal(tok, torch.cat([ta, tb], 0))
    assert torch.equal(lp.cpu().view(torch.int32), torch.cat([la, lb], 0).cpu().view(torch.int32))
    # trimmed: a chunk that ends earlier than the widest one is zero-filled
    sched_t = torch.tensor([1] * 14 + [4] * 6, dtype=torch.int32, device=backend)
    tt, lt = m.generate(**_inputs(b, rows20, alias20), **dict(kw, eos_schedule=sched_t, return_full_length=False))
    assert tt.shape == lt.shape == (20, 5) and bool((lt[:14, 2:] == 0.0).all()) and bool((tt[:14, 2:] == 1).all())
    monkeypatch.setenv("BRA_DEC_ROWS32", "1")
    if generation._one_loop_ok(m.text_model, 20):
        seen.clear()
        t1, l1 = m.generate(**_inputs(b, rows20, alias20), **kw)
        assert seen == [] and t1.shape == l1.shape == (20, T)
        after = _zeros_after_eos(t1, l1, eos)
        assert bool(after.any()) and bool((l1.cpu()[~after & (t1.cpu() != eos)] < 0).any())
    else:
        print("\n[rollout-logp] no 32-row forms at the fixture's widths: one-loop half not run")


def test_processors_are_refused_before_any_launch(backend, monkeypatch):
    """each processor clash raises a ValueError that names it, before any launch (not one call into the kernel library)"""
    fix, m, b = _tiny_b(backend)
    tm = m.text_model
    emb = torch.zeros((2, 6, fix["config"]["text"]["hidden_size"]), dtype=torch.bfloat16, device=backend)
    mask = torch.ones((2, 6), dtype=torch.long, device=backend)
    calls = []
    lib = get_lib()
    real = lib.call
    monkeypatch.setattr(lib, "call", lambda *a, **k: calls.append(a[0]) or real(*a, **k))
    clashes = {"repetition_penalty": dict(repetition_penalty=1.2), "min_new_tokens": dict(min_new_tokens=2, eos_token_id=5),
               "no_repeat_ngram_size": dict(no_repeat_ngram_size=2), "bad_words_ids": dict(bad_words_ids=[[7]]),
               "suppress_tokens": dict(suppress_tokens=[3]), "begin_suppress_tokens": dict(begin_suppress_tokens=[3]),
               "sequence_bias": dict(sequence_bias={(9,): -1.0})}
    for name, kw in clashes.items():
        with pytest.raises(ValueError, match=name):
            generation.generate(tm, emb, mask, max_new_tokens=4, return_logprobs=True, **kw)
    assert calls == []
    # the warpers are fine, and so is every processor at its neutral value
    tok, lp = generation.generate(tm, emb, mask, max_new_tokens=4, return_logprobs=True, do_sample=True, temperature=0.7, top_k=20, top_p=0.9,
                                  min_p=0.05, repetition_penalty=1.0, min_new_tokens=0, no_repeat_ngram_size=0)
    assert tok.shape == lp.shape == (2, 4) and calls
    with pytest.raises(ValueError, match="repetition_penalty"):
        m.generate(**_inputs(b, [0, 1]), max_new_tokens=4, return_logprobs=True, repetition_penalty=1.3)


# ------------------------------------------------------------------------------------------------------------------- the step runner
EPS, EPS_HIGH = 0.2, 0.3                # (the clamp edges of tests/test_grpo_loss_is.py, whose float64 oracle is used below)


def _runner_batch(fix, dev, copies=2):
    from test_shared_policy import _group_batch
    ids, mask, mm, alias = _group_batch(fix, dev, copies)
    return {"input_ids": ids, "attention_mask": mask, "dna_tokenized": mm["dna_tokenized"], "batch_idx_map": mm["batch_idx_map"],
            "prompt_alias": alias}


def _loss_with_capture(runner, batch, monkeypatch):
    """one rollout + compute_loss + backward -> (inputs dict, the arguments grpo.grpo_loss saw, stats, d loss / d logp)"""
    seen = {}
    real = grpo.grpo_loss

    def spy(logp, old, ref, adv, mask, eps_lo, eps_hi, beta, **kw):
        logp.retain_grad()
        seen.update(logp=logp, old=old, ref=ref, adv=adv, mask=mask, eps=(eps_lo, eps_hi), beta=beta, kw=kw)
        return real(logp, old, ref, adv, mask, eps_lo, eps_hi, beta, **kw)
    monkeypatch.setattr(grpo, "grpo_loss", spy)
    inputs = runner.generate_and_score(batch)
    runner.model.arena.zero_grad()
    loss, stats = runner.compute_loss(inputs)
    loss.backward()
    monkeypatch.setattr(grpo, "grpo_loss", real)
    return inputs, seen, stats.detach().cpu(), seen["logp"].grad.detach().cpu()


def _oracle_check(seen, stats, grad, cap, label):
    """the float64 oracle of tests/test_grpo_loss_is.py fed the recorded tensors: loss, statistics and the gradient on logp"""
    from test_grpo_loss_is import _ratio, _reference, _twin_worst
    f = lambda t_: None if t_ is None else t_.detach().float().cpu()
    assert seen["eps"] == (EPS, EPS_HIGH)
    rl = f(seen["kw"]["rollout_logp"])
    r = _reference(f(seen["logp"]), f(seen["old"]), f(seen["ref"]), f(seen["adv"]), seen["mask"].detach().cpu().to(torch.int32), rl, seen["beta"], cap)
    ratios = {"dlogp": _ratio((grad.to(F64) - r["dlogp"]).abs(), r["E"]), "loss": abs(stats[0].item() - r["loss"]) / r["E_loss"],
              "is_mean": abs(stats[3].item() - r["is_mean"]) / r["E_is"],
              "rollout_kl": abs(stats[5].item() - r["rollout_kl"]) / r["E_rkl"] if r["E_rkl"] > 0 else 0.0}
    print(f"\n[rollout-logp] {label}: is_mean {stats[3].item():.6f} is_capped {stats[4].item():.6f} rollout_kl {stats[5].item():.3e} | "
          + " ".join(f"{k_} {v_:.3f}" for k_, v_ in ratios.items()))
    assert ratios["dlogp"] <= 2 * _twin_worst(), ratios
    assert ratios["loss"] <= 1.0 and ratios["is_mean"] <= 1.0 and ratios["rollout_kl"] <= 1.0, ratios
    assert abs(stats[4].item() - r["is_capped"]) <= 4 * U32 * max(r["is_capped"], 1e-30)
    return r


def test_grpo_step_with_rollout_is_correction_bf16(backend, monkeypatch):
    from test_model_parity import build
    from bioreason_amd.trainer import GRPOConfig, GRPOStepRunner
    fix = torch.load(os.path.join(GOLD, "tiny_b.pt"), weights_only=False)
    common = dict(num_generations=2, max_completion_length=6, eos_token_id=None, seed=3, learning_rate=1e-3, temperature=20.0,
                  epsilon=EPS, epsilon_high=EPS_HIGH)
    cap = 2.0
    # one whole step runs and reports the three extra metrics
    m = build(fix, backend, True)
    runner = GRPOStepRunner(m, GRPOConfig(**common, rollout_is_correction=True, rollout_is_cap=cap))
    assert runner.metric_names[-3:] == ["is_mean", "is_capped", "rollout_kl"]
    out = runner.step(_runner_batch(fix, backend))
    buf = runner._buffered_inputs[0]
    assert buf["rollout_per_token_logps"].shape == buf["completion_ids"].shape and buf["rollout_per_token_logps"].dtype == F32
    met = dict(zip(runner.metric_names, out["metrics_t"].tolist()))
    assert len(out["metrics_t"]) == 9 and 0.0 < met["is_mean"] <= cap and 0.0 <= met["is_capped"] <= 1.0
    assert torch.isfinite(out["metrics_t"]).all() and torch.isfinite(out["loss_t"]).all()
    # the loss's arguments, recorded, against the float64 oracle
    m = build(fix, backend, True)
    runner = GRPOStepRunner(m, GRPOConfig(**common, rollout_is_correction=True, rollout_is_cap=cap))
    inputs, seen, stats, grad = _loss_with_capture(runner, _runner_batch(fix, backend), monkeypatch)
    assert inputs["rollout_per_token_logps"] is seen["kw"]["rollout_logp"] and seen["kw"]["is_cap"] == cap
    assert torch.equal(inputs["rollout_per_token_logps"].cpu(), buf["rollout_per_token_logps"].cpu())      # same seed, same rollout
    assert stats.shape == (6,) and 0.0 < stats[3].item() <= cap and math_isfinite(stats[5].item())
    _oracle_check(seen, stats, grad, cap, "bf16 rollout, tiny_b")
    # the flag off: the call of before — no keyword to generate(), three statistics, no entry in the metrics
    m = build(fix, backend, True)
    runner0 = GRPOStepRunner(m, GRPOConfig(**common))
    gen_kw = {}
    real_gen = m.generate
    monkeypatch.setattr(m, "generate", lambda **k: gen_kw.update(k) or real_gen(**k))
    inputs0, seen0, stats0, grad0 = _loss_with_capture(runner0, _runner_batch(fix, backend), monkeypatch)
    assert "return_logprobs" not in gen_kw and inputs0["rollout_per_token_logps"] is None and seen0["kw"] == {} and stats0.shape == (3,)
    assert torch.equal(inputs0["completion_ids"], inputs["completion_ids"])
    assert runner0.metric_names == GRPOStepRunner.metric_names and len(GRPOStepRunner.metric_names) == 6
    # configuration errors surface when the runner is constructed
    for bad, word in ((dict(rollout_is_cap=0.5), "rollout_is_cap"), (dict(repetition_penalty=1.1), "repetition_penalty"),
                      (dict(no_repeat_ngram_size=2), "no_repeat_ngram_size"), (dict(bad_words_ids=[[3]]), "bad_words_ids"),
                      (dict(suppress_tokens=[3]), "suppress_tokens")):
        with pytest.raises(ValueError, match=word):
            GRPOStepRunner(m, GRPOConfig(**common, rollout_is_correction=True, **bad))
    GRPOStepRunner(m, GRPOConfig(**common, repetition_penalty=1.1))           # (without the correction the processors stay allowed)


def math_isfinite(v):
    import math
    return math.isfinite(v)


# the smallest widths the fp8 row forms accept (tests/test_fp8_rows16.py MIXED: Wqkv, Wo, Wgu and the lm_head stream e4m3, the down
# projection — K = 1280 — its bf16 packed image), behind the fixture's DNA encoder
FP8_TEXT = dict(vocab_size=2048, hidden_size=1024, intermediate_size=1280, num_hidden_layers=1, num_attention_heads=8, num_key_value_heads=2,
                head_dim=128, rope_theta=1e6, max_position_embeddings=4096)


def _fp8_model(fix, dev):
    from bioreason_amd import configs
    from bioreason_amd.dna_llm import DNALLMModel
    d = fix["config"]["dna"]
    dc = configs.nt_v2_config(**{k: d[k] for k in ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads",
                                                   "max_position_embeddings")})
    m = DNALLMModel(configs.qwen3_config(**FP8_TEXT), dc, device=dev, dna_token_id=fix["config"]["dna_token_id"])
    m.text_model.init_weights(0.02, seed=1)
    m.dna_model.init_weights(0.05, seed=2)
    m.text_model.apply_lora(r=32, alpha=64.0, dropout=0.0, arena=m.arena)
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for n_, p_ in m.text_model.named_parameters():
            if "lora_B" in n_:                                   # (a trained adapter: B != 0, so the merged weights differ from the base)
                p_.copy_((0.02 * torch.randn(p_.shape, generator=g)).to(p_.dtype).to(dev))
        m.dna_projection.weight.copy_((0.02 * torch.randn(m.dna_projection.weight.shape, generator=g)).to(dev))
        m.dna_projection.bias.zero_()
    m.arena.pack()
    return m


@pytest.mark.gpu
def test_grpo_step_with_rollout_is_correction_fp8(hip_device, monkeypatch):
    """rollout_fp8 at widths whose projections stream e4m3: the corrected loss and gradient differ from the uncorrected step's and match
    the float64 oracle fed the recorded tensors"""
    from bioreason_amd.trainer import GRPOConfig, GRPOStepRunner
    dev = hip_device
    fix = torch.load(os.path.join(GOLD, "tiny_b.pt"), weights_only=False)
    common = dict(num_generations=2, max_completion_length=6, eos_token_id=None, seed=3, learning_rate=1e-3, temperature=1.0,
                  epsilon=EPS, epsilon_high=EPS_HIGH, rollout_fp8=True)
    cap = 2.0
    res = {}
    for on in (True, False):
        m = _fp8_model(fix, dev)
        runner = GRPOStepRunner(m, GRPOConfig(**common, rollout_is_correction=on, rollout_is_cap=cap))
        inputs, seen, stats, grad = _loss_with_capture(runner, _runner_batch(fix, dev), monkeypatch)
        m.text_model.rollout_fp8 = True
        rw = generation.rollout_weights(m.text_model, rows=inputs["completion_ids"].shape[0])
        assert all(tuple(R.get("fp8_proj", ())) == ("Wqkv", "Wo", "Wgu") for R in rw), "the rollout did not stream e4m3 images"
        res[on] = (inputs, seen, stats, grad)
    (i1, s1, st1, g1), (i0, s0, st0, g0) = res[True], res[False]
    assert torch.equal(i1["completion_ids"], i0["completion_ids"])              # the same rollout
    assert torch.equal(s1["logp"].detach().cpu(), s0["logp"].detach().cpu())    # the same policy pass
    assert st1.shape == (6,) and st0.shape == (3,)
    assert st1[0].item() != st0[0].item() and not torch.equal(g1, g0)
    assert 0.0 < st1[3].item() <= cap and math_isfinite(st1[5].item())
    _oracle_check(s1, st1, g1, cap, "fp8 rollout (Wqkv, Wo, Wgu, lm_head e4m3)")
