"""The entropy metric and bonus above the kernels: grpo.grpo_loss(entropy=..., entropy_coef=...), GRPOStepRunner with log_entropy /
entropy_coef, DNALLMGRPOConfig / DNALLMGRPOTrainer.

grpo_loss.  The returned loss is  loss_kernel - entropy_coef * mean_b( sum_c(ent mask) / sum_c(mask) )  — the reference's normalisation
(grpo_trainer.py:801-803) applied to per_token_loss - entropy_coef H — and stats gains one trailing entry, that mean.  Held against a
float64 statement written here (oracle/grpo_math.grpo_loss for the kernel's part, tests/test_grpo_loss_is.py's statement with the
importance weight): the bonus is three fp32 torch statements over C terms per row, so
    |entropy stat - ref|  <=  u (C + B + 3) mean_b( sum_c |ent| mask / sum_c mask ),      u = 2^-24
(a sum of C products, the division, the mean over B rows: worst case, ratio <= 1 without a margin), the loss within that times
entropy_coef plus the kernel's own loss bound and one rounding of the difference, d loss / d ent = -entropy_coef mask / (ms B) within
3 u relative, and dlogp is the kernel's, bit for bit (the bonus does not touch it).  A row whose mask is all zero is 0 / 0 in the
reference's statement, in the loss kernel and in the bonus alike: NaN in, NaN out, on both sides.

GRPOStepRunner on the tiny model of the runner tests (tests/golden/tiny_b.pt), as tests/test_rollout_logprobs.py proceeds for its switch.
"""
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bioreason_amd import grpo, ops                                    # noqa: E402
from oracle import grpo_math                                           # noqa: E402
from test_grpo_loss_is import EPS_LO, EPS_HI, _edges, _inputs, _reference      # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")
F32, F64 = torch.float32, torch.float64
U32 = 2.0 ** -24
COEF = 0.01


def _entropy(B, C):
    """fp32 [B, C] in [0, ln 151936): what a policy's per-token entropy looks like, with exact zeros (a collapsed token)"""
    g = torch.Generator().manual_seed(7 * B + C)
    ent = torch.rand(B, C, generator=g) * 11.9
    ent.view(-1)[4::9] = 0.0
    return ent


def _bonus_ref(ent, mask):
    m = mask.to(F64)
    ms = m.sum(1)
    e = ent.to(F64)
    B, C = ent.shape
    mean = ((e * m).sum(1) / ms).mean()
    bound = U32 * (C + B + 3) * ((e.abs() * m).sum(1) / ms).mean()
    dent = m / (ms[:, None] * B)
    return mean.item(), bound.item(), dent


# (B, C, old_logp given, rollout_logp given)
LOSS_CASES = [(1, 1, False, False), (4, 255, True, False), (4, 257, False, True), (8, 700, True, True), (8, 700, False, False)]


@pytest.mark.parametrize("B,C,use_old,use_rl", LOSS_CASES)
def test_grpo_loss_with_entropy(backend, B, C, use_old, use_rl):
    dev = backend
    beta, cap = 0.04, 2.0
    lp, old, ref, adv, mask, rl = _inputs(B, C, use_old, cap)
    ent = _entropy(B, C)
    kw = dict(rollout_logp=rl.to(dev), is_cap=cap) if use_rl else {}
    n0 = 6 if use_rl else 3

    def call(**extra):
        lpd = lp.to(dev).clone().requires_grad_(True)
        entd = ent.to(dev).clone().requires_grad_(True)
        if "entropy" in extra:
            extra["entropy"] = entd
        loss, stats = grpo.grpo_loss(lpd, old.to(dev) if old is not None else None, ref.to(dev), adv.to(dev), mask.to(dev), EPS_LO, EPS_HI,
                                     beta, **kw, **extra)
        loss.backward()
        return loss.detach().cpu(), stats.detach().cpu(), lpd.grad.cpu(), None if entd.grad is None else entd.grad.cpu()

    loss0, stats0, dlp0, _ = call()
    loss1, stats1, dlp1, dent1 = call(entropy=True, entropy_coef=COEF)
    lossz, statsz, dlpz, dentz = call(entropy=True, entropy_coef=0.0)
    assert stats0.shape == (n0,) and stats1.shape == (n0 + 1,) and statsz.shape == (n0 + 1,)
    # entropy_coef = 0: the loss and dlogp of the call without `entropy`, bit for bit; the entropy receives no gradient
    assert torch.equal(lossz.view(torch.int32), loss0.view(torch.int32)) and torch.equal(dlpz.view(torch.int32), dlp0.view(torch.int32))
    assert dentz is None
    # the existing positions are unchanged, the bonus does not touch dlogp
    assert torch.equal(stats1[:n0].view(torch.int32), stats0.view(torch.int32)) and torch.equal(statsz.view(torch.int32), stats1.view(torch.int32))
    assert torch.equal(dlp1.view(torch.int32), dlp0.view(torch.int32))
    # against float64: the kernel's part by the oracle of tests/test_grpo_loss_is.py (w = 1 when there is no rollout_logp: q itself)
    r = _reference(lp, old, ref, adv, mask, rl if use_rl else (old if old is not None else lp), beta, cap if use_rl else 1e30)
    mean, bound, dent_ref = _bonus_ref(ent, mask)
    e_stat = abs(stats1[n0].item() - mean) / bound
    want = r["loss"] - COEF * mean
    e_loss = abs(loss1.item() - want) / (r["E_loss"] + COEF * bound + U32 * abs(want))
    e_dent = ((dent1.to(F64) + COEF * dent_ref).abs() / (3 * U32 * COEF * dent_ref).clamp_min(1e-300))[mask.bool()].max().item()
    print(f"\n[grpo-entropy] B{B} C{C} {'old' if use_old else 'noold'} {'is' if use_rl else 'plain'}: stat {e_stat:.3f} loss {e_loss:.3f} dent {e_dent:.3f}")
    assert e_stat <= 1.0 and e_loss <= 1.0 and e_dent <= 1.0
    assert (dent1[mask == 0] == 0).all()


def test_grpo_loss_with_entropy_all_zero_mask_row(backend):
    """a row without a live token: 0 / 0 in the reference's normalisation — the float64 statement, the kernel's loss and the bonus agree
    (NaN), and the live rows' gradients are the ones of the float64 statement"""
    dev = backend
    B, C, beta = 4, 257, 0.04
    lp, old, ref, adv, mask, _ = _inputs(B, C, True, 2.0)
    mask = mask.clone()
    mask[1] = 0
    ent = _entropy(B, C)
    lo, hi = _edges()
    l64, _, _ = grpo_math.grpo_loss(lp.to(F64), old.to(F64), ref.to(F64), adv.to(F64), mask.to(F64), 1 - lo, hi - 1, beta)
    mean64 = ((ent.to(F64) * mask.to(F64)).sum(1) / mask.to(F64).sum(1)).mean()
    assert math.isnan(l64.item()) and math.isnan(mean64.item())
    entd = ent.to(dev).clone().requires_grad_(True)
    lpd = lp.to(dev).clone().requires_grad_(True)
    loss, stats = grpo.grpo_loss(lpd, old.to(dev), ref.to(dev), adv.to(dev), mask.to(dev), EPS_LO, EPS_HI, beta, entropy=entd, entropy_coef=COEF)
    assert math.isnan(loss.item()) and math.isnan(stats[0].item()) and math.isnan(stats[3].item())
    loss.backward()
    live = mask.bool()
    _, _, dent_ref = _bonus_ref(ent, mask)
    got = entd.grad.cpu().to(F64)
    assert ((got + COEF * dent_ref).abs()[live] <= 3 * U32 * COEF * dent_ref[live]).all()
    assert (lpd.grad.cpu()[1] == 0).all()                              # (the kernel writes 0 for a row without a live token)


def test_grpo_loss_entropy_coef_is_validated(backend):
    lp, old, ref, adv, mask, _ = _inputs(4, 255, True, 2.0)
    a = [t.to(backend) for t in (lp, old, ref, adv, mask)]
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="entropy_coef"):
            grpo.grpo_loss(*a, EPS_LO, EPS_HI, 0.04, entropy=_entropy(4, 255).to(backend), entropy_coef=bad)


# ------------------------------------------------------------------------------------------------------------------- the step runner
EPS, EPS_HIGH = 0.2, 0.3
COMMON = dict(num_generations=2, max_completion_length=3, eos_token_id=None, seed=3, learning_rate=1e-3, temperature=20.0,
              epsilon=EPS, epsilon_high=EPS_HIGH)


def _fix():
    return torch.load(os.path.join(GOLD, "tiny_b.pt"), weights_only=False)


def _flat_model(fix, dev):
    """tiny_b's top logit leads by ~30 (its entropy is ~1e-6: nothing for a bonus to move), so the tests that need a policy with
    entropy run the fixture's batch through a randomly initialised text model of the same vocabulary behind the fixture's DNA encoder
    configuration (entropy near ln V), with trained-looking adapters (lora_B != 0)"""
    from bioreason_amd import configs
    from bioreason_amd.dna_llm import DNALLMModel
    d = fix["config"]["dna"]
    dc = configs.nt_v2_config(**{k: d[k] for k in ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads",
                                                   "max_position_embeddings")})
    tc = configs.qwen3_config(vocab_size=fix["config"]["text"]["vocab_size"], hidden_size=64, intermediate_size=128, num_hidden_layers=2,
                              num_attention_heads=4, num_key_value_heads=2, head_dim=32, rope_theta=1e6, max_position_embeddings=512)
    m = DNALLMModel(tc, dc, device=dev, dna_token_id=fix["config"]["dna_token_id"])
    m.text_model.init_weights(0.25, seed=1)
    m.dna_model.init_weights(0.05, seed=2)
    m.text_model.apply_lora(r=32, alpha=64.0, dropout=0.0, arena=m.arena)
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for n_, p_ in m.text_model.named_parameters():
            if "lora_B" in n_:
                p_.copy_((0.02 * torch.randn(p_.shape, generator=g)).to(p_.dtype).to(dev))
        m.dna_projection.weight.copy_((0.02 * torch.randn(m.dna_projection.weight.shape, generator=g)).to(dev))
        m.dna_projection.bias.zero_()
    m.arena.pack()
    m.train()
    return m


def _runner(fix, dev, flat=False, **over):
    from test_model_parity import build
    from bioreason_amd.trainer import GRPOConfig, GRPOStepRunner
    m = _flat_model(fix, dev) if flat else build(fix, dev, True)
    return m, GRPOStepRunner(m, GRPOConfig(**{**COMMON, **over}))


def _batch(fix, dev):
    from test_rollout_logprobs import _runner_batch
    return _runner_batch(fix, dev)


@pytest.mark.parametrize("flat", [False, True])
def test_log_entropy_adds_the_metric_and_changes_no_update(backend, flat):
    """log_entropy alone: the parameters after a step are the bits of the step without it, the six metrics too; `entropy` is appended
    (tiny_b, and the model with entropy)"""
    fix = _fix()
    V = fix["config"]["text"]["vocab_size"]
    m0, r0 = _runner(fix, backend, flat)
    out0 = r0.step(_batch(fix, backend))
    m1, r1 = _runner(fix, backend, flat, log_entropy=True)
    seen = []
    real = ops.lmhead_dlogits
    ops.lmhead_dlogits = lambda *a, **k: seen.append(len(a) + len(k)) or real(*a, **k)
    try:
        out1 = r1.step(_batch(fix, backend))
    finally:
        ops.lmhead_dlogits = real
    assert seen == [5]                                                 # a metric nobody differentiates: the old dlogits launch
    assert r0.metric_names == type(r0).metric_names and r1.metric_names == type(r0).metric_names + ["entropy"]
    assert torch.equal(m1.arena.params, m0.arena.params)
    assert len(out0["metrics_t"]) == 6 and len(out1["metrics_t"]) == 7
    assert torch.equal(out1["metrics_t"][:6], out0["metrics_t"]) and torch.equal(out1["loss_t"], out0["loss_t"])
    ent = out1["metrics_t"][6].item()
    print(f"\n[grpo-entropy] {'random-init model' if flat else 'tiny_b'} (V = {V}, ln V = {math.log(V):.4f}): entropy {ent:.3e}")
    assert 0.0 < ent <= math.log(V) * (1 + 1e-6)
    if flat:
        assert ent > 0.5 * math.log(V)


def test_entropy_metric_shared_and_full_row_pass(backend):
    """The shared-prompt and the full-row policy pass report the same entropy to the tolerance their log-probs agree to (0.06,
    tests/test_shared_policy.py: bf16 activations, rounding placed differently); with the importance-sampling statistics the entry
    lands behind them."""
    fix = _fix()
    V = fix["config"]["text"]["vocab_size"]
    m1, r1 = _runner(fix, backend, True, log_entropy=True)
    ent_shared = r1.step(_batch(fix, backend))["metrics_t"][6].item()
    m2, r2 = _runner(fix, backend, True, log_entropy=True, share_policy_prompt=False)
    out2 = r2.step(_batch(fix, backend))
    ent_full = out2["metrics_t"][6].item()
    print(f"\n[grpo-entropy] random-init model (V = {V}, ln V = {math.log(V):.4f}): entropy {ent_shared:.5f} shared-prompt pass, {ent_full:.5f} full-row pass")
    assert 0.5 * math.log(V) < ent_shared <= math.log(V) and abs(ent_shared - ent_full) < 0.06
    m3, r3 = _runner(fix, backend, True, log_entropy=True, rollout_is_correction=True)
    out3 = r3.step(_batch(fix, backend))
    assert r3.metric_names[-4:] == ["is_mean", "is_capped", "rollout_kl", "entropy"] and len(out3["metrics_t"]) == 10
    assert torch.isfinite(out3["metrics_t"]).all() and out3["metrics_t"][9].item() == ent_shared        # (the same rollout, the same policy pass)


def _restated_loss(coef):
    """float32 torch restatement of the step's loss with the bonus (autograd does the rest): what grpo.grpo_loss is replaced by"""
    def loss_fn(logp, old, ref, adv, mask, eps_lo, eps_hi, beta, rollout_logp=None, is_cap=2.0, entropy=None, entropy_coef=0.0):
        assert entropy is not None and entropy_coef == coef
        one = torch.tensor(1.0, dtype=F32, device=logp.device)
        lo, hi = one - torch.tensor(eps_lo, dtype=F32, device=logp.device), one + torch.tensor(eps_hi, dtype=F32, device=logp.device)
        q = old if old is not None else logp.detach()
        A = adv.float()[:, None]
        c1 = torch.exp(logp - q)
        ptl = -torch.min(c1 * A, torch.minimum(torch.maximum(c1, lo), hi) * A)
        if rollout_logp is not None:
            ptl = torch.clamp(torch.exp(q - rollout_logp), max=is_cap) * ptl
        tot = ptl - entropy_coef * entropy
        if beta:
            d = ref - logp
            tot = tot + beta * (torch.exp(d) - d - 1)
        mk = mask.float()
        loss = ((tot * mk).sum(1) / mk.sum(1)).mean()
        n = 6 if rollout_logp is not None else 3
        return loss, torch.cat([loss.detach().reshape(1), torch.zeros(n, device=logp.device)])
    return loss_fn


@pytest.mark.parametrize("shared,is_corr", [(True, False), (False, False), (True, True)])
def test_entropy_coef_changes_the_update_and_matches_a_restatement(backend, monkeypatch, shared, is_corr):
    """entropy_coef > 0: one dlogits launch carries both coefficients; the arena gradient of the step's loss equals the arena gradient of
    a float32 torch restatement of that loss (clipped objective + beta k3 - entropy_coef H, the reference's normalisation) pushed through
    the same policy pass.  The two differ by fp32 roundings of dlogp / dent only, which move a bf16 dlogits element by at most one
    rounding: relative difference <= 2 U = 2^-8 in the Frobenius norm, U = 2^-9."""
    from test_model_parity import rel
    fix = _fix()
    over = dict(entropy_coef=0.05, share_policy_prompt=shared, rollout_is_correction=is_corr)

    def grads(patch):
        m, r = _runner(fix, backend, True, **over)
        if patch:
            monkeypatch.setattr(grpo, "grpo_loss", _restated_loss(0.05))
        seen = []
        real = ops.lmhead_dlogits
        monkeypatch.setattr(ops, "lmhead_dlogits", lambda *a, **k: seen.append(len(a) + len(k)) or real(*a, **k))
        inputs = r.generate_and_score(_batch(fix, backend))
        m.arena.zero_grad()
        loss, stats = r.compute_loss(inputs)
        loss.backward()
        monkeypatch.undo()
        assert seen == [7]
        return loss.item(), stats.detach().cpu(), m.arena.grads.clone(), inputs["completion_ids"].clone()

    l_k, stats, g_k, ids_k = grads(False)
    l_t, _, g_t, ids_t = grads(True)
    assert torch.equal(ids_k, ids_t)                                    # same seed, same rollout
    n = 6 if is_corr else 3
    assert stats.shape == (n + 1,) and abs(l_k - (stats[0].item() - 0.05 * stats[n].item())) <= 4 * U32 * (abs(stats[0].item()) + stats[n].item())
    d = rel(g_k, g_t)
    print(f"\n[grpo-entropy] shared={shared} is={is_corr}: loss {l_k:.6f} / restated {l_t:.6f}, entropy {stats[n].item():.5f}, arena gradient rel {d:.2e}")
    assert abs(l_k - l_t) <= 1e-5 * max(1.0, abs(l_t))
    assert d <= 2.0 ** -8
    # and the bonus does change the update: against the same step with the metric only
    m0, r0 = _runner(fix, backend, True, log_entropy=True, share_policy_prompt=shared, rollout_is_correction=is_corr)
    inputs0 = r0.generate_and_score(_batch(fix, backend))
    m0.arena.zero_grad()
    r0.compute_loss(inputs0)[0].backward()
    assert torch.equal(inputs0["completion_ids"], ids_k) and rel(g_k, m0.arena.grads) > 1e-3


def test_entropy_under_iterations_and_accumulation(backend):
    """num_iterations = 2 and gradient_accumulation_steps = 2: buffered rollouts and old log-probs; every micro-batch reports a finite entropy, the optimiser
    steps report the seven metrics"""
    fix = _fix()
    V = fix["config"]["text"]["vocab_size"]
    m, r = _runner(fix, backend, True, entropy_coef=0.01, num_iterations=2, gradient_accumulation_steps=2)
    p0 = m.arena.params.clone()
    outs = [r.step(_batch(fix, backend)) for _ in range(4)]
    assert r.global_step == 2 and r.step_idx == 2
    for o in outs:
        assert torch.isfinite(o["loss_t"]).all() and o["stats_t"].shape == (4,) and 0.0 < o["stats_t"][3].item() <= math.log(V) * (1 + 1e-6)
    assert "metrics_t" not in outs[0] and len(outs[1]["metrics_t"]) == 7 and torch.isfinite(outs[3]["metrics_t"]).all()
    assert (m.arena.params - p0).abs().max() > 0


def test_entropy_coef_is_validated_at_construction(backend):
    from bioreason_amd.trainer import GRPOConfig, GRPOStepRunner
    from bioreason_amd.grpo_trainer import DNALLMGRPOConfig
    from types import SimpleNamespace
    for bad in (-0.01, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="entropy_coef"):
            GRPOConfig(entropy_coef=bad)
        with pytest.raises(ValueError, match="entropy_coef"):
            DNALLMGRPOConfig(output_dir="/tmp/_cfg", report_to="none", entropy_coef=bad)
    c = GRPOConfig()
    assert c.log_entropy is False and c.entropy_coef == 0.0
    import numpy
    for ok in (numpy.float32(0.01), torch.tensor(0.01), 0, 1):          # (a sweep script's scalar types are numbers too)
        GRPOConfig(entropy_coef=ok)
    with pytest.raises(ValueError, match="entropy_coef"):
        GRPOConfig(entropy_coef="a lot")
    a = DNALLMGRPOConfig(output_dir="/tmp/_cfg", report_to="none")
    assert a.log_entropy is False and a.entropy_coef == 0.0
    assert DNALLMGRPOConfig(output_dir="/tmp/_cfg", report_to="none", entropy_coef=0.01, log_entropy=True).entropy_coef == 0.01
    # a config object assembled by hand is checked where the runner reads it
    fix = _fix()
    from test_model_parity import build
    m = build(fix, backend, True)
    cfg = GRPOConfig(**COMMON)
    cfg.entropy_coef = -1.0
    with pytest.raises(ValueError, match="entropy_coef"):
        GRPOStepRunner(m, cfg)
    assert GRPOStepRunner(m, GRPOConfig(**COMMON, entropy_coef=0.01)).with_entropy          # entropy_coef > 0 implies the metric


@pytest.fixture
def emulator(emu_lib_path):
    """host-logic tests run on the kernel-source emulator alone"""
    from bioreason_amd import _lib
    _lib.use_library_for_tests(emu_lib_path)
    yield torch.device("cpu")
    _lib.reset_library()


def test_trainer_logs_entropy(emulator, tmp_path):
    """DNALLMGRPOTrainer with log_entropy: `entropy` is logged where kl and clip_ratio are"""
    backend = emulator
    from test_grpo_trainer import _toy_tokenizers
    from bioreason.dna_modules import NucleotideDNAModule
    from bioreason.trainer import DNALLMGRPOConfig, DNALLMGRPOTrainer
    from bioreason_amd import configs, rewards
    from bioreason_amd.chat_template import CHAT_TEMPLATE
    from bioreason_amd.dna_llm import DNALLMModel
    tc = configs.qwen3_config(vocab_size=256, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
                              num_key_value_heads=2, head_dim=32, max_position_embeddings=512)
    dc = configs.nt_v2_config(vocab_size=16, hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2,
                              max_position_embeddings=64)
    tok, dtok = _toy_tokenizers(tmp_path, 256)
    tok.chat_template = CHAT_TEMPLATE
    m = DNALLMModel(tc, dc, device=backend, dna_token_id=tok.convert_tokens_to_ids("<|dna_pad|>"))
    m.text_model.init_weights(0.05, seed=1)
    m.dna_model.init_weights(0.05, seed=2)
    m.text_tokenizer, m.dna_tokenizer, m.max_length_text, m.max_length_dna = tok, dtok, 64, 16
    data = [{"prompt": [{"role": "user", "content": [{"type": "dna"}, {"type": "text", "text": f"Which pathway w{20 + i} ?"}]}],
             "dna_sequences": ["ACGTAC" + "GT" * i], "answer": "ALS"} for i in range(2)]
    args = DNALLMGRPOConfig(output_dir=str(tmp_path / "out"), report_to="none", per_device_train_batch_size=2, num_generations=2,
                            max_completion_length=4, learning_rate=1e-3, logging_steps=1, save_strategy="no", max_steps=2, seed=3,
                            use_cpu=True, log_entropy=True, entropy_coef=0.01)
    tr = DNALLMGRPOTrainer(model=m, reward_funcs=[rewards.xmlcount_reward_func], args=args, dna_module=NucleotideDNAModule(),
                           train_dataset=data, peft_config={"r": 32, "lora_alpha": 64, "lora_dropout": 0.0})
    assert tr.runner.with_entropy and tr.runner.entropy_coef == 0.01
    tr.train()
    assert len(tr.log_history) == 2
    for k in ("kl", "clip_ratio", "entropy"):
        assert k in tr.log_history[-1], k
    assert 0.0 < tr.log_history[-1]["entropy"] <= math.log(256) * (1 + 1e-6)
