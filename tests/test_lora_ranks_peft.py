"""The public seam at other adapter ranks: `get_peft_model(text_model, LoraConfig(r, lora_alpha, lora_dropout, ...))` through
`compat/peft`, as reason.py:376-388 / train_dna_qwen.py:155-167 call it with `--lora_rank` and `--lora_dropout` — one SFT step in
training mode (dropout active) must move every adapter tensor.  See tests/test_peft_seam.py for the seam itself."""
import importlib.util
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TARGETS = ["q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"]


def _shim():
    spec = importlib.util.spec_from_file_location("peft_shim_under_test", os.path.join(ROOT, "compat", "peft", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _tiny(backend):
    from test_model_parity import GOLD, build
    fix = torch.load(os.path.join(GOLD, "tiny_b.pt"), weights_only=False)
    return build(fix, backend, False), fix


@pytest.mark.parametrize("r", [16, 64])
def test_get_peft_model_with_dropout_at_other_ranks_trains(backend, r):
    from bioreason_amd.trainer import SFTStepRunner
    from test_model_parity import to_dev
    shim = _shim()
    m, fix = _tiny(backend)
    cfg = shim.LoraConfig(r=r, lora_alpha=2 * r, lora_dropout=0.1, target_modules=TARGETS, init_lora_weights="gaussian")
    m.text_model = shim.get_peft_model(m.text_model, cfg)
    assert m.text_model.lora_dropout_p == pytest.approx(0.1)
    before = {n: p.detach().clone() for n, p in m.named_parameters() if "lora_" in n}
    assert len(before) == 14 * len(m.text_model.model.layers)
    assert all(p.shape[0 if "lora_A" in n else 1] == r for n, p in before.items())
    m.train()
    runner = SFTStepRunner(m, learning_rate=1e-2, weight_decay=0.0)
    batch = to_dev(fix["batch"], backend)
    assert torch.isfinite(runner.step(batch)["loss_t"]).item()
    # B starts at zero (gaussian init): the first step can only move B, the second moves A through the B it made
    now = dict(m.named_parameters())
    assert all(not torch.equal(now[n].detach(), v) for n, v in before.items() if "lora_B" in n)
    assert torch.isfinite(runner.step(batch)["loss_t"]).item()
    now = dict(m.named_parameters())
    still = [n for n, v in before.items() if torch.equal(now[n].detach(), v)]
    assert not still, still


def test_dropout_at_a_rank_without_a_masked_kernel_is_refused(backend):
    m, _ = _tiny(backend)
    with pytest.raises(NotImplementedError) as e:
        m.text_model.apply_lora(r=40, dropout=0.05, arena=m.arena)
    assert all(str(r) in str(e.value) for r in (8, 16, 32, 64, 128))
