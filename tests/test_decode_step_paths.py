"""The fallback branches of the fused decode step's driver (k_decode.hip: step_gemms / sg_qkv / sg_tail / sg_head) that real shapes
reach when the packer refuses a projection, when the hidden size needs more than 256 statistics columns, or when the lm_head
stays unpacked: selected here by the host switches BRA_DEC_PACK=0 (plain-layout bra_dec_gemm2), BRA_DEC_GEMM_V1=1
(first-generation bra_dec_gemm, no statistics workspace) and BRA_DEC_PACK_HEAD=0 (plain lm_head), each against the default
(packed + folded) path, on the per-sequence step (FusedDecodeState) and on the shared-prefix step (SharedDecodeState, attention
"one").  tiny_b (H = 256, hd = 128, Hq / Hkv = 2 / 1, F = 512, V = 384, L = 1) is the smallest fixture that takes the packed and
folded path and the shared-prefix step.

Two statements per case:
  (a) the built state took the intended path: the `flags` word of layer record 0 (bit 0 packed, bit 1 norms folded, bit 2 head
      folded) and the statistics columns `nss` — a host decision, so the same numbers on the emulator and on the device;
  (b) teacher-forced with the reference's greedy tokens, the choices equal the default path's except in near-ties of the reference's
      own fp32 scores — the criterion of test_model_parity.py::test_fused_decode_step_matches_unfused: a differing position needs
      |score[a] - score[c]| < 0.02 max|score| + 0.05, and there are at most 2 of them.
Measured, emulator and MI355X alike: 0 differing tokens in all six cases; the logits differ from the default path's by at most
0.17 (BRA_DEC_PACK=0 / BRA_DEC_GEMM_V1=1) and 0.06 (BRA_DEC_PACK_HEAD=0) at a largest logit of 44.4."""
import os

import pytest
import torch

from bioreason_amd import generation
from test_model_parity import build, to_dev

GOLD = os.path.join(os.path.dirname(__file__), "golden")
ROWS = [0, 0, 1, 1]
ALIASES = {"fused": None, "shared": [0, 0, 2, 2]}
STATE = {"fused": "FusedDecodeState", "shared": "SharedDecodeState"}
# switch -> (flags of layer record 0, nss) of the state it must build; the default path: (7, 32)
SWITCHES = {"BRA_DEC_PACK=0": (0, 32), "BRA_DEC_PACK_HEAD=0": (3, 32), "BRA_DEC_GEMM_V1=1": (0, 0)}
DEFAULT = (7, 32)

_fix = {}
_default = {}          # (device type, step) -> (tokens, [(flags, nss)]) of the default path, computed once


def _fixture():
    if not _fix:
        _fix["tiny_b"] = torch.load(os.path.join(GOLD, "tiny_b.pt"), weights_only=False)
    return _fix["tiny_b"]


def _run(dev, step):
    """teacher-forced greedy decode of the four rows -> (tokens on the host, [(flags, nss)] of every state the call built)"""
    fix = _fixture()
    cfg = fix["config"]
    m = build(fix, dev, True)
    b = to_dev(fix["batch"], dev)
    ids, mask = b["input_ids"][ROWS], b["attention_mask"][ROWS]
    dna = {k: v[ROWS] for k, v in b["dna_tokenized"].items()}       # one DNA sequence per sample in tiny_b
    mm = {"dna_tokenized": dna, "batch_idx_map": [0, 1, 2, 3]}
    want = fix["fp32_lora"]["greedy_ids"][ROWS].to(dev)
    seen = []
    with pytest.MonkeyPatch.context() as mp:            # (the states' constructors are wrapped for this call only)
        for name in STATE.values():
            cls = getattr(generation, name)

            def spy(self, *a, _orig=cls.__init__, _name=name, **k):
                _orig(self, *a, **k)
                seen.append((_name, getattr(self, "attn_impl", None), int(self.arr[0].flags), int(self.nss)))
            mp.setattr(cls, "__init__", spy)
        extra = {} if ALIASES[step] is None else {"prompt_alias": ALIASES[step]}
        toks = m.generate(input_ids=ids, attention_mask=mask, **mm, **extra, max_new_tokens=cfg["gen_tokens"], do_sample=False,
                          eos_token_id=None, force_tokens=want)
    assert [s[0] for s in seen] == [STATE[step]], seen
    if step == "shared":
        assert seen[0][1] == "one", seen
    return toks.cpu(), [s[2:] for s in seen]


@pytest.mark.parametrize("switch", list(SWITCHES))
@pytest.mark.parametrize("step", list(ALIASES))
def test_driver_fallback_branch_decodes_what_the_default_path_decodes(backend, monkeypatch, step, switch):
    for name in ("BRA_DEC_PACK", "BRA_DEC_PACK_HEAD", "BRA_DEC_GEMM_V1", "BRA_DEC_ATTN"):
        monkeypatch.delenv(name, raising=False)
    key = (backend.type, step)
    if key not in _default:
        _default[key] = _run(backend, step)
    g_d, path_d = _default[key]
    assert path_d == [DEFAULT], path_d
    name, value = switch.split("=")
    monkeypatch.setenv(name, value)
    g_s, path_s = _run(backend, step)
    assert path_s == [SWITCHES[switch]], (switch, path_s)
    scores = _fixture()["fp32_lora"]["greedy_scores"][ROWS]
    diff = (g_d != g_s).nonzero().tolist()
    print(f"{backend.type} {step} {switch}: {len(diff)} differing tokens {diff}")
    for bi, t in diff:
        a, c = int(g_d[bi, t]), int(g_s[bi, t])
        assert abs((scores[bi, t, a] - scores[bi, t, c]).item()) < 0.02 * scores[bi, t].abs().max().item() + 0.05, (bi, t, a, c)
    assert len(diff) <= 2, diff
