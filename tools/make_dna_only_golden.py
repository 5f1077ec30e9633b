"""Writes tests/golden/dna_only.pt: what the reference's DNA-only head computes on fixed hidden states (CPU, build container only).

    python tools/make_dna_only_golden.py

The reference classes are imported at run time from the reference checkout; nothing of their text is kept.  The file holds tensors
and names only: a tiny encoder config, bf16 hidden states and masks for ref / alt, labels, the head's state_dict, the reference's
float64 logits and parameter gradients (CrossEntropyLoss, eval mode), and the same quantities from the reference run in bf16.
"""
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG = dict(vocab_size=16, hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2, max_position_embeddings=256)
B, S_REF, S_ALT, C = 3, 140, 133, 2


def reference_head(Pool, H, C, state, dtype):
    pool, clf = Pool(H), nn.Sequential(nn.Linear(2 * H, H), nn.ReLU(), nn.Dropout(0.1), nn.Linear(H, C))
    pool.load_state_dict({k[len("pooler."):]: v for k, v in state.items() if k.startswith("pooler.")}, strict=True)
    clf.load_state_dict({k[len("classifier."):]: v for k, v in state.items() if k.startswith("classifier.")}, strict=True)
    return pool.to(dtype), clf.to(dtype)


def run_reference(Pool, H, C, state, fix, dtype, train=False, seed=None):
    """-> (logits, {state_dict key: grad}) of the reference classes in `dtype`"""
    pool, clf = reference_head(Pool, H, C, state, dtype)
    pool.train(train), clf.train(train)
    if seed is not None:
        torch.manual_seed(seed)
    ref = pool(fix["ref_h"].to(dtype), fix["ref_mask"])
    alt = pool(fix["alt_h"].to(dtype), fix["alt_mask"])
    logits = clf(torch.cat([ref, alt], dim=1))
    nn.CrossEntropyLoss()(logits.float() if dtype == torch.bfloat16 else logits, fix["labels"]).backward()
    grads = {"pooler." + k: p.grad for k, p in pool.named_parameters()}
    grads.update({"classifier." + k: p.grad for k, p in clf.named_parameters()})
    return logits.detach(), grads


def main():
    from oracle.make_golden import import_from_reference
    from bioreason_amd.dna_only import SelfAttentionPooling
    Pool = import_from_reference("bioreason.models.dna_only", "SelfAttentionPooling")
    H = CFG["hidden_size"]
    g = torch.Generator().manual_seed(11)
    fix = {"config": dict(CFG),
           "ref_h": torch.randn(B, S_REF, H, generator=g).to(torch.bfloat16), "alt_h": torch.randn(B, S_ALT, H, generator=g).to(torch.bfloat16),
           "ref_mask": torch.ones(B, S_REF, dtype=torch.long), "alt_mask": torch.ones(B, S_ALT, dtype=torch.long),
           "labels": torch.tensor([0, 1, 1])}
    fix["ref_mask"][0, 100:] = 0
    fix["ref_mask"][1, :130] = 0            # left padding past the first 128-row chunk
    fix["alt_mask"][2, 40:90] = 0
    torch.manual_seed(12)
    pool = SelfAttentionPooling(H)
    clf = nn.Sequential(nn.Linear(2 * H, H), nn.ReLU(), nn.Dropout(0.1), nn.Linear(H, C))
    state = {"pooler." + k: v.detach().clone() for k, v in pool.state_dict().items()}
    state.update({"classifier." + k: v.detach().clone() for k, v in clf.state_dict().items()})
    state["pooler.attention.in_proj_bias"] = 0.1 * torch.randn(3 * H, generator=g)      # torch initialises it to zero
    fix["state_dict"] = state
    fix["logits64"], fix["grads64"] = run_reference(Pool, H, C, state, fix, torch.float64)
    fix["logits_bf16"], gb = run_reference(Pool, H, C, state, fix, torch.bfloat16)
    fix["grads_bf16"] = {k: v.float() for k, v in gb.items()}
    out = os.path.join(ROOT, "tests", "golden", "dna_only.pt")
    torch.save(fix, out)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
