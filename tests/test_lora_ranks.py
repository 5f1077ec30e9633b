"""LoRA at every adapter rank (`lora_r` / `--lora_rank` and `--lora_dropout` of the reference scripts, train_dna_qwen.py:1036-1038,
reason.py:264-266): the masked kernels for r = 8 ... 128 (one mask stream per TARGET module, whatever the rank; target j = rank
columns [j r, (j + 1) r) of the fused group), the plain branch for fused groups wider than 128 rank columns, and the model under
dropout against the oracle with the same masks injected.  The peft entry is in test_lora_ranks_peft.py."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bioreason_amd import ops                            # noqa: E402
from bioreason_amd._lib import BRA_ERR_ARG, KernelError, current_stream, get_lib  # noqa: E402

BF = torch.bfloat16


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def rnd(*shape, dev, scale=1.0, seed=None):
    g = torch.Generator().manual_seed(seed if seed is not None else sum(shape) + len(shape))
    return (torch.randn(*shape, generator=g) * scale).to(BF).to(dev)


def r_pad(r, targets):
    return (targets * r + 63) // 64 * 64                 # engine.LoraGroup


RANK_CASES = [(8, 1), (8, 3), (16, 2), (16, 3), (32, 1), (32, 2), (32, 3), (32, 4), (64, 1), (64, 3), (128, 2), (128, 3)]
P, SEEDS = 0.25, [5, 6, 7, 8]


def _operands(r, targets, M, K, dev):
    """x, the group's A image and dts in the LoraGroup layout (padding rows / columns past targets * r are zeros), and per target the
    exported mask and torch's dropout of x under it (scale in fp32, one rounding to bf16)"""
    R = r_pad(r, targets)
    x, A, dts = rnd(M, K, dev=dev), rnd(R, K, dev=dev, scale=K ** -0.5), rnd(M, R, dev=dev)
    A[targets * r:] = 0
    dts[:, targets * r:] = 0
    masks = [ops.dropout_mask(M, K, P, SEEDS[j], dev).float().cpu() for j in range(targets)]
    xd = [(x.float().cpu() * mk / (1 - P)).to(BF).float() for mk in masks]
    return x, A, dts, masks, xd


def _want_t(A, xd, r, targets, M):
    want = torch.zeros(M, A.shape[0])
    for j in range(targets):
        want[:, j * r:(j + 1) * r] = 0.5 * xd[j] @ A.float().cpu()[j * r:(j + 1) * r].T
    return want


def _want_dA(dts, xd, r, targets, K):
    want = torch.zeros(dts.shape[1], K)
    for j in range(targets):
        want[j * r:(j + 1) * r] = dts.float().cpu()[:, j * r:(j + 1) * r].T @ xd[j]
    return want


# ----------------------------------------------------------------------------- 1. kernels, injected masks
@pytest.mark.parametrize("r,targets", RANK_CASES)
def test_lora_dropout_kernels_at_every_rank(backend, r, targets):
    """forward t = s drop_j(x) A_j^T, input gradient sum_j drop_j'(dts_j A_j) and weight gradient dA_j += dts_j^T drop_j(x) with target
    j = rank columns [j r, (j + 1) r) and mask stream seeds[j] — against fp32 torch under the exported masks.  M = 97: four 32-row
    blocks, ragged; K = 136: two 128-wide K steps, ragged.  A wrong column -> seed map fails the bounds below by two orders of
    magnitude (masks of different seeds agree on (1-p)^2 + p^2 of the elements only)."""
    M, K = 97, 136
    seeds = SEEDS[:targets]
    x, A, dts, masks, xd = _operands(r, targets, M, K, backend)
    R = A.shape[0]
    t = ops.lora_down_drop(x, A, 0.5, P, seeds, rank=r)
    assert rel(t, _want_t(A, xd, r, targets, M).to(BF)) < 4e-3
    assert (t[:, targets * r:] == 0).all()
    up = ops.lora_up_drop(dts, A.T.contiguous(), P, seeds, rank=r)
    want_up = sum((dts.float().cpu()[:, j * r:(j + 1) * r] @ A.float().cpu()[j * r:(j + 1) * r]) * masks[j] / (1 - P)
                  for j in range(targets))
    assert rel(up, want_up.to(BF)) < 4e-3
    dA = torch.zeros(R, K, device=backend)
    ops.wgrad_tn(x, dts, dA, transposed_out=True, drop=(P, seeds), rank=r)
    assert rel(dA, _want_dA(dts, xd, r, targets, K)) < 1e-5 and (dA[targets * r:] == 0).all()


@pytest.mark.parametrize("r,targets", RANK_CASES)
def test_lora_down_drop_split_k_at_every_rank(backend, r, targets):
    """K = 776 at M = 97: bra_lora_down_splitk_plan says 2, so the split-K form runs (fp32 partial tiles per slice of the group, summed in
    a fixed order): same masks, same bound, deterministic"""
    M, K = 97, 776
    seeds = SEEDS[:targets]
    assert get_lib()._dll.bra_lora_down_splitk_plan(M, K) == 2
    x, A, _, _, xd = _operands(r, targets, M, K, backend)
    old = ops.LORA_DOWN_SPLITK
    try:
        ops.LORA_DOWN_SPLITK = True
        t1 = ops.lora_down_drop(x, A, 0.5, P, seeds, rank=r)
        t2 = ops.lora_down_drop(x, A, 0.5, P, seeds, rank=r)
    finally:
        ops.LORA_DOWN_SPLITK = old
    assert torch.equal(t1.cpu(), t2.cpu())
    assert rel(t1, _want_t(A, xd, r, targets, M).to(BF)) < 4e-3 and (t1[:, targets * r:] == 0).all()


@pytest.mark.parametrize("r,targets", RANK_CASES)
def test_wgrad_drop_row_chunks_at_every_rank(backend, r, targets):
    """M = 300 with m_chunk = 64: five row chunks per column tile meet in C through atomics"""
    M, K = 300, 136
    seeds = SEEDS[:targets]
    x, A, dts, _, xd = _operands(r, targets, M, K, backend)
    dA = torch.zeros(A.shape[0], K, device=backend)
    ops.wgrad_tn(x, dts, dA, transposed_out=True, m_chunk=64, drop=(P, seeds), rank=r)
    assert rel(dA, _want_dA(dts, xd, r, targets, K)) < 1e-5 and (dA[targets * r:] == 0).all()


def test_ranks_without_a_masked_kernel_are_refused(backend):
    x, A = rnd(8, 64, dev=backend), rnd(128, 64, dev=backend)
    with pytest.raises(NotImplementedError, match="128"):
        ops.lora_down_drop(x, A, 1.0, 0.1, [1, 2, 3], rank=40)


def test_group_descriptions_outside_the_contract_are_refused(backend):
    """the C entry points themselves (include/bioreason_hip.h: r in {8, 16, 32, 64, 128}; r = 32: 1 <= nt <= R / 32; otherwise
    1 <= nt <= 3 and R = ceil(nt r / 64) 64; split-K needs `part`): BRA_ERR_ARG from all three, and nothing is launched — the outputs
    keep their fill"""
    M, K = 8, 256
    lib, st = get_lib(), current_stream(None)

    def status(name, *args):
        try:
            return lib.call(name, *args)
        except KernelError as e:
            return e.status
    for r, nt, R in [(32, 0, 64), (32, 3, 64), (16, 4, 64), (64, 3, 128), (40, 1, 64)]:
        x, A, dts = rnd(M, K, dev=backend), rnd(R, K, dev=backend), rnd(M, R, dev=backend)
        t, up = torch.full((M, R), 7.0, dtype=BF, device=backend), torch.full((M, K), 7.0, dtype=BF, device=backend)
        dA = torch.full((R, K), 7.0, device=backend)
        part = torch.full((2, M, R), 7.0, device=backend)
        for ks in (1, 2):
            assert status("bra_lora_down_drop", x, K, A, K, t, R, M, K, R, 0.5, P, *SEEDS, r, nt, part, ks, st) == BRA_ERR_ARG, (r, nt, R)
        assert status("bra_lora_up_drop", dts, R, A.T.contiguous(), R, up, K, M, K, R, P, *SEEDS, r, nt, st) == BRA_ERR_ARG, (r, nt, R)
        assert status("bra_wgrad_tn_drop", x, K, dts, R, dA, 1, K, M, K, R, 1.0, 0, P, *SEEDS, r, nt, st) == BRA_ERR_ARG, (r, nt, R)
        assert (t == 7).all() and (up == 7).all() and (dA == 7).all() and (part == 7).all()
    # a valid group (32 x 2 in 64 columns; ksplit = 2 <= ceil(K / 128)), split-K without the partial tiles
    x, A, t = rnd(M, K, dev=backend), rnd(64, K, dev=backend), torch.full((M, 64), 7.0, dtype=BF, device=backend)
    assert status("bra_lora_down_drop", x, K, A, K, t, 64, M, K, 64, 0.5, P, *SEEDS, 32, 2, None, 2, st) == BRA_ERR_ARG
    assert (t == 7).all()
    assert status("bra_lora_down_drop", x, K, A, K, t, 64, M, K, 64, 0.5, P, *SEEDS, 32, 2, None, 1, st) == 0     # the plain form
    assert not (t == 7).all()


# ----------------------------------------------------------------------------- 2. the plain branch past 128 rank columns
@pytest.mark.parametrize("r,n_targets", [(64, 3), (128, 2), (128, 3), (48, 3)])
def test_lora_branch_without_dropout_past_128_rank_columns(backend, r, n_targets):
    """test_kernels.py::test_lora_branch_without_dropout_at_any_rank at group widths 192 / 256 / 384 (r = 64 and 128 over q/k/v or
    gate/up; r = 48 x 3 = 144 -> 192): the weight gradients of engine._lora_bwd need bra_wgrad_tn at any multiple of 64 columns"""
    from bioreason_amd.engine import QwenEngine
    M, K, Nj = 70, 96, 64
    rp = r_pad(r, n_targets)
    assert rp > 128
    x, W = rnd(M, K, dev=backend), rnd(n_targets * Nj, K, dev=backend, scale=K ** -0.5)
    A = torch.zeros(rp, K, dtype=BF, device=backend)
    B_ = torch.zeros(n_targets * Nj, rp, dtype=BF, device=backend)
    for j in range(n_targets):
        A[j * r:(j + 1) * r] = rnd(r, K, dev=backend, scale=K ** -0.5, seed=j + 1)
        B_[j * Nj:(j + 1) * Nj, j * r:(j + 1) * r] = rnd(Nj, r, dev=backend, scale=0.3, seed=j + 9)

    class G:                                            # the fields of engine.LoraGroup the branch reads
        pass
    G.A, G.AT, G.B, G.BT = A, A.T.contiguous(), B_, B_.T.contiguous()
    G.scaling, G.n_sizes, G.r = 2.0, [Nj] * n_targets, r
    G.A_grad = torch.zeros(rp, K, device=backend)
    G.B_grad = torch.zeros(n_targets * Nj, rp, device=backend)
    y, t = QwenEngine._lora_fwd(x, W, G, True)
    t_ref = 2.0 * (x.float() @ A.float().T)
    assert rel(t, t_ref) < 4e-3
    y_ref = x.float() @ W.float().T + t_ref.to(BF).float() @ B_.float().T
    assert rel(y, y_ref) < 6e-3
    dy = rnd(M, n_targets * Nj, dev=backend, seed=77)
    dx = QwenEngine._lora_bwd(dy, W.T.contiguous(), G, True, x, t)
    dts_ref = 2.0 * (dy.float() @ B_.float())
    dx_ref = dy.float() @ W.float() + dts_ref.to(BF).float() @ A.float()
    assert rel(dx, dx_ref) < 6e-3
    assert rel(G.A_grad, dts_ref.to(BF).float().T @ x.float()) < 6e-3
    assert rel(G.B_grad, dy.float().T @ t.float()) < 6e-3


# ----------------------------------------------------------------------------- 3. the model under dropout, oracle with the same masks
class _FixedMask(torch.nn.Module):
    """stands in for a LoraLayer's nn.Dropout with a given keep mask: x * mask / (1 - p)"""

    def __init__(self, mask, p):
        super().__init__()
        self.mask, self.p = mask, p

    def forward(self, x):
        return x * self.mask.to(x.dtype).view(x.shape) / (1.0 - self.p)


@pytest.mark.parametrize("r", [8, 16, 64])
@pytest.mark.parametrize("name", ["tiny_a", "tiny_b"])
def test_lora_dropout_matches_oracle_at_other_ranks(backend, name, r):
    """test_edge_cases.py::test_lora_dropout_matches_oracle_under_the_same_masks at r = 8, 16 (several targets in one 32-column rank
    block) and 64 (a target over two blocks, q/k/v = 192 columns): adapters filled with seeded values (B non-zero), the masks the
    kernels regenerate exported and injected into the oracle"""
    from bioreason_amd.engine import lora_drop_seeds
    from oracle import dna_llm_oracle as O
    from test_model_parity import GOLD, build, to_dev
    from test_oracle import rebuild
    p = 0.2
    fix = torch.load(os.path.join(GOLD, f"{name}.pt"), weights_only=False)
    b = fix["batch"]
    m = build(fix, backend, False)
    m.text_model.apply_lora(r=r, alpha=2.0 * r, dropout=p, arena=m.arena)
    own = dict(m.text_model.named_parameters())
    gen = torch.Generator().manual_seed(1000 + r)
    values = {}
    for k in sorted(k for k in own if "lora_" in k):
        std = 1.0 / r if "lora_A" in k else 0.05
        values[k] = (torch.randn(own[k].shape, generator=gen) * std).to(BF).float()
        own[k].data.copy_(values[k].to(backend))
    assert values
    m.arena.pack()
    m.train()
    m.text_model.set_dropout_seed(123)
    pass_seed = (123 * 0x9E3779B1 + 1 * 0x85EBCA6B) & 0xFFFFFFFF            # first forward after set_dropout_seed

    def oracle():
        ora = rebuild(fix, False)
        O.apply_lora(ora.text_model, r=r, alpha=2.0 * r)
        missing, unexpected = ora.text_model.load_state_dict(values, strict=False)
        assert not unexpected and not [k for k in missing if "lora_" in k]
        return ora
    ora = oracle()
    B, S = b["input_ids"].shape
    where = {"q_proj": ("qkv", 0, 3), "k_proj": ("qkv", 1, 3), "v_proj": ("qkv", 2, 3), "o_proj": ("o", 0, 1),
             "gate_proj": ("gu", 0, 2), "up_proj": ("gu", 1, 2), "down_proj": ("d", 0, 1)}
    injected = 0
    for li, layer in enumerate(ora.text_model.model.layers):
        for holder in (layer.self_attn, layer.mlp):
            for nm, (grp, j, n) in where.items():
                mod = getattr(holder, nm, None)
                if isinstance(mod, O.LoraLinear):
                    K = mod.base_layer.in_features
                    seed = lora_drop_seeds(pass_seed, li, grp, n)[j]
                    mod.dropout = _FixedMask(ops.dropout_mask(B * S, K, p, seed, backend).cpu().view(B, S, K), p)
                    injected += 1
    assert injected == 7 * len(ora.text_model.model.layers)
    want = ora(**{k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()})
    want.loss.backward()
    m.arena.zero_grad()
    got = m(**to_dev(b, backend))
    keep = b["attention_mask"].bool()
    tol = 2.5e-2
    assert rel(got.logits.float().cpu()[keep], want.logits.detach()[keep]) < tol
    assert abs(got.loss.item() - want.loss.item()) < tol * max(1.0, abs(want.loss.item()))
    got.loss.backward()
    assert rel(m.dna_projection.weight.grad, ora.dna_projection.weight.grad) < 3 * tol
    l0, r0 = m.text_model.model.layers[0], ora.text_model.model.layers[0]
    for nm, mod, ref in (("q", l0.self_attn.q_proj, r0.self_attn.q_proj), ("k", l0.self_attn.k_proj, r0.self_attn.k_proj),
                         ("up", l0.mlp.up_proj, r0.mlp.up_proj), ("down", l0.mlp.down_proj, r0.mlp.down_proj)):
        assert rel(mod.lora_A["default"].weight.grad, ref.lora_A["default"].weight.grad) < 3 * tol, nm
        assert rel(mod.lora_B["default"].weight.grad, ref.lora_B["default"].weight.grad) < 3 * tol, nm
    # the masks matter: without them the oracle's gradients are measurably different (guards against a silent no-op)
    ora2 = oracle()
    w2 = ora2(**{k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()})
    w2.loss.backward()
    assert rel(r0.mlp.down_proj.lora_A["default"].weight.grad, ora2.text_model.model.layers[0].mlp.down_proj.lora_A["default"].weight.grad) > 0.1
    # eval mode: no dropout (nn.Dropout is the identity)
    m.eval()
    ev = m(**to_dev(b, backend))
    assert rel(ev.logits.float().cpu()[keep], w2.logits.detach()[keep]) < tol
