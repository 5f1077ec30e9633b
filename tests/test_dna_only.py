"""DNAClassifierModel / SelfAttentionPooling (bioreason_amd/dna_only.py) against the reference's DNA-only head.

Criterion as in tests/test_attn_pool.py: per row (logits: per example; gradients: per row of each parameter) the relative L2 error
against the reference classes in float64 must be <= 1.25 x the error of the reference classes run in bf16, floored at its median.
"""
import os
import subprocess
import sys
import types

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_attn_pool import worst_ratio  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "dna_only.pt")
HAVE_REF = os.path.exists("/root/reference/bioreason/models/dna_only.py")
needs_ref = pytest.mark.skipif(not HAVE_REF, reason="reference checkout not present (its source text is never copied into this repository)")
TINY = dict(vocab_size=16, hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2, max_position_embeddings=256)


def as2d(t):
    return t.reshape(-1, t.shape[-1]) if t.dim() > 1 else t.reshape(1, -1)


def our_head(state, dev, C=2):
    from bioreason_amd.dna_only import SelfAttentionPooling
    H = state["pooler.query"].shape[-1]
    pool = SelfAttentionPooling(H)
    clf = nn.Sequential(nn.Linear(2 * H, H), nn.ReLU(), nn.Dropout(0.1), nn.Linear(H, C))
    pool.load_state_dict({k[7:]: v for k, v in state.items() if k.startswith("pooler.")}, strict=True)
    clf.load_state_dict({k[11:]: v for k, v in state.items() if k.startswith("classifier.")}, strict=True)
    return pool.to(dev), clf.to(dev)


def run_ours(state, fix, dev, train=False, seed=None):
    pool, clf = our_head(state, dev)
    pool.train(train), clf.train(train)
    if seed is not None:
        torch.manual_seed(seed)
    ref = pool(fix["ref_h"].to(dev), fix["ref_mask"].to(dev))
    alt = pool(fix["alt_h"].to(dev), fix["alt_mask"].to(dev))
    logits = clf(torch.cat([ref, alt], dim=1))
    nn.CrossEntropyLoss()(logits, fix["labels"].to(dev)).backward()
    grads = {"pooler." + k: p.grad.cpu() for k, p in pool.named_parameters()}
    grads.update({"classifier." + k: p.grad.cpu() for k, p in clf.named_parameters()})
    return logits.detach().cpu(), grads


def check(tag, logits, grads, l64, g64, lbf, gbf):
    H = g64["pooler.query"].shape[-1]
    worst = {"logits": worst_ratio(logits, lbf, l64)}
    for k in g64:
        ours, yard, truth = grads[k], gbf[k].float(), g64[k]
        if k == "pooler.attention.in_proj_bias":
            # the key bias cancels in the softmax: exactly 0 here, rounding noise in the reference
            assert float(ours[H:2 * H].abs().max()) == 0.0
            assert float(truth[H:2 * H].abs().max()) < 1e-12
            sel = torch.cat([torch.arange(0, H), torch.arange(2 * H, 3 * H)])
            ours, yard, truth = ours[sel], yard[sel], truth[sel]
        worst[k] = worst_ratio(as2d(ours), as2d(yard), as2d(truth))
    print(f"dna_only {tag}: worst ratios " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if not v <= 1.25}
    assert not bad, bad


def test_head_matches_the_recorded_reference(backend):
    """reads only tests/golden/dna_only.pt (tools/make_dna_only_golden.py): runs on the GPU machine, where no reference exists"""
    fix = torch.load(GOLD, weights_only=False)
    logits, grads = run_ours(fix["state_dict"], fix, backend)
    check("golden", logits, grads, fix["logits64"], fix["grads64"], fix["logits_bf16"], fix["grads_bf16"])


@needs_ref
@pytest.mark.parametrize("train", [False, True])
def test_head_matches_the_reference_classes(emu_lib_path, train):
    from bioreason_amd import _lib
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_dna_only_golden as M
    from oracle.make_golden import import_from_reference
    Pool = import_from_reference("bioreason.models.dna_only", "SelfAttentionPooling")
    fix = torch.load(GOLD, weights_only=False)
    state, H = fix["state_dict"], fix["config"]["hidden_size"]
    M.reference_head(Pool, H, 2, state, torch.float32)                          # strict load: keys and shapes equal the reference's
    from bioreason_amd.dna_only import SelfAttentionPooling
    assert {k: tuple(v.shape) for k, v in Pool(H).state_dict().items()} == {k: tuple(v.shape) for k, v in SelfAttentionPooling(H).state_dict().items()}
    l64, g64 = M.run_reference(Pool, H, 2, state, fix, torch.float64, train, seed=3)
    lbf, gbf = M.run_reference(Pool, H, 2, state, fix, torch.bfloat16, train, seed=3)
    _lib.use_library_for_tests(emu_lib_path)
    try:
        logits, grads = run_ours(state, fix, torch.device("cpu"), train, seed=3)
    finally:
        _lib.reset_library()
    check("train" if train else "eval", logits, grads, l64, g64, lbf, gbf)


def tiny_model(dev, **kw):
    from bioreason_amd import configs
    from bioreason_amd.dna_only import DNAClassifierModel
    torch.manual_seed(4)
    m = DNAClassifierModel(configs.nt_v2_config(**TINY), device=dev, **kw)
    m.dna_model.init_weights(0.05, seed=2)
    return m


def test_batched_forward_equals_one_example_at_a_time_and_adamw_moves_the_head(backend):
    m = tiny_model(backend).eval()
    g = torch.Generator().manual_seed(6)
    B, Sr, Sa = 3, 140, 70
    ref_ids, alt_ids = torch.randint(4, 16, (B, Sr), generator=g).to(backend), torch.randint(4, 16, (B, Sa), generator=g).to(backend)
    rm, am = torch.ones(B, Sr, dtype=torch.long), torch.ones(B, Sa, dtype=torch.long)
    rm[0, 90:], rm[1, 133:], am[2, 50:] = 0, 0, 0
    rm, am = rm.to(backend), am.to(backend)
    logits = m(ref_ids, alt_ids, rm, am)
    assert logits.shape == (B, 2) and logits.dtype == torch.float32
    alone = torch.cat([m(ref_ids[i:i + 1], alt_ids[i:i + 1], rm[i:i + 1], am[i:i + 1]) for i in range(B)])
    # the same kernels on the same rows: batching changes neither the encoder's nor the pooling's arithmetic per row
    assert torch.allclose(logits, alone, rtol=1e-5, atol=1e-6), (logits - alone).abs().max()
    m.train()
    enc_before = [p.detach().clone() for p in m.dna_model.parameters()]
    head_before = {k: p.detach().clone() for k, p in m.named_parameters() if k.startswith(("pooler.", "classifier."))}
    opt = torch.optim.AdamW(m.parameters(), lr=1e-2)
    nn.CrossEntropyLoss()(m(ref_ids, alt_ids, rm, am), torch.tensor([0, 1, 1], device=backend)).backward()
    opt.step()
    H = m.hidden_size
    now = dict(m.named_parameters())
    w0, w1 = head_before["pooler.attention.in_proj_weight"], now["pooler.attention.in_proj_weight"]
    for blk in range(3):
        assert not torch.equal(w0[blk * H:(blk + 1) * H], w1[blk * H:(blk + 1) * H]), blk
    for k in ("pooler.query", "pooler.attention.out_proj.weight", "classifier.0.weight", "classifier.3.weight"):
        assert not torch.equal(head_before[k], now[k]), k
    for p, q in zip(m.dna_model.parameters(), enc_before):
        assert torch.equal(p, q) and not p.requires_grad


def test_refusals():
    from bioreason_amd import configs
    from bioreason_amd.dna_only import DNAClassifierModel
    with pytest.raises(NotImplementedError, match="backward"):
        DNAClassifierModel(configs.nt_v2_config(**TINY), train_just_classifier=False, device="cpu")
    with pytest.raises(ImportError, match="evo2"):
        DNAClassifierModel("evo2_1b_base", dna_is_evo2=True, dna_embedding_layer="blocks.2", device="cpu")


class Evo2StandIn:
    """Evo2's call interface over a fixed embedding table (one sequence per call: no `supports_batch`)"""

    def __init__(self, H=64):
        self.table = torch.randn(32, H, generator=torch.Generator().manual_seed(8))
        self.model = types.SimpleNamespace(config=types.SimpleNamespace(hidden_size=H))
        self.tokenizer, self.calls = None, 0

    def __call__(self, input_ids, return_embeddings=False, layer_names=None):
        self.calls += 1
        assert input_ids.shape[0] == 1
        return None, {layer_names[0]: self.table.to(input_ids.device)[input_ids]}


def test_evo2_stand_in_on_left_padded_input_and_1d_ids(backend):
    from bioreason_amd.dna_only import DNAClassifierModel
    enc = Evo2StandIn()
    torch.manual_seed(9)
    m = DNAClassifierModel(enc, dna_is_evo2=True, dna_embedding_layer="blocks.2", device=backend).eval()
    ids = torch.randint(1, 32, (2, 150), generator=torch.Generator().manual_seed(10))
    mask = torch.ones(2, 150, dtype=torch.long)
    mask[0, :131], mask[1, :7] = 0, 0
    emb = m.get_dna_embedding(ids.to(backend), mask.to(backend))
    assert emb.shape == (2, 64) and enc.calls == 2
    # float64 statement of the pooling over the same bf16 hidden states
    x = enc.table[ids].to(torch.bfloat16).double()
    att = m.pooler.attention
    W, bias = att.in_proj_weight.detach().cpu().double(), att.in_proj_bias.detach().cpu().double()
    q = (W[:64] @ m.pooler.query.detach().cpu().double().reshape(64) + bias[:64]).view(8, 8)
    k = (x @ W[64:128].T + bias[64:128]).view(2, 150, 8, 8)
    v = (x @ W[128:].T + bias[128:]).view(2, 150, 8, 8)
    s = torch.einsum("hd,nlhd->nhl", q, k) * 8 ** -0.5
    p = torch.softmax(s.masked_fill(mask[:, None, :] == 0, float("-inf")), -1)
    ctx = torch.einsum("nhl,nlhd->nhd", p, v).reshape(2, 64)
    want = ctx @ att.out_proj.weight.detach().cpu().double().T + att.out_proj.bias.detach().cpu().double()
    err = (emb.detach().cpu().double() - want).norm(dim=1) / want.norm(dim=1)
    assert float(err.max()) < 1e-4, err                       # fp32 arithmetic over H = 64, S = 150: far inside bf16's 2^-9
    one = m.get_dna_embedding(ids[1].to(backend), mask[1].to(backend))
    assert one.shape == (64,) and torch.allclose(one, emb[1], rtol=1e-5, atol=1e-6)
    assert m.get_dna_embedding(ids[1].to(backend), None).shape == (64,)


def test_train_dna_only_imports_resolve_in_a_fresh_interpreter():
    code = ("from bioreason.models.dna_only import DNAClassifierModel\n"
            "from bioreason.dataset.utils import truncate_dna\n"
            "from bioreason.dataset.kegg import dna_collate_fn\n"
            "from bioreason.dataset.variant_effect import clean_variant_effect_example\n"
            "from bioreason.models.evo2_tokenizer import Evo2Tokenizer, register_evo2_tokenizer\n"
            "import bioreason_amd.dna_only as d\n"
            "assert DNAClassifierModel is d.DNAClassifierModel\n")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT, env={**os.environ, "PYTHONPATH": ROOT})
