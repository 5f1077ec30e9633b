"""The reference's DNA-only baseline (bioreason/models/dna_only.py) on the HIP encoder.

``DNAClassifierModel`` keeps the reference's constructor, attribute names and ``state_dict`` keys for ``pooler.*`` and
``classifier.*``.  What differs is where the work happens:

* the frozen encoder is ``NTEncoderForMaskedLM`` (HIP), called once per side over the whole batch instead of 2 B times;
* ``SelfAttentionPooling`` never calls its ``nn.MultiheadAttention``.  With one learned, input-independent query the K and V
  projections fold into the query (DESIGN.md "Attention pooling"), and the data-sized work is ``ops.attn_pool_fwd`` /
  ``ops.attn_pool_bwd`` — one pass over the hidden states each;
* the parameter-sized math around the kernels (the folded query, the per-head ``W_v``, ``out_proj``, the classifier) stays plain
  fp32 torch under autograd: a deliberate, bounded exception to "no torch compute on the product path" (under 20 MFLOP per step
  at B = 8) that keeps the reference's dropout stream and gives ``W_q`` / ``W_k`` / ``query`` their gradients for free.
"""
from __future__ import annotations

from typing import Any, Optional, Union

import torch
import torch.nn as nn

from . import ops

BF16 = torch.bfloat16


class _AttnPoolFn(torch.autograd.Function):
    """pooled [n, 8, H] = sum_l softmax_l(x_l . qt_h) x_l around the two kernels; the hidden states are frozen: no gradient for x"""

    @staticmethod
    def forward(ctx, x, mask, qt):
        qt = qt.detach().contiguous()
        pooled, lse = ops.attn_pool_fwd(x, mask, qt)
        ctx.save_for_backward(x, mask, qt, pooled, lse)
        return pooled

    @staticmethod
    def backward(ctx, g):
        x, mask, qt, pooled, lse = ctx.saved_tensors
        return None, None, ops.attn_pool_bwd(x, mask, qt, pooled, lse, g.contiguous().float())


class SelfAttentionPooling(nn.Module):
    """dna_only.py:8-39.  `attention` holds the parameters under the reference's names and is never called."""

    def __init__(self, hidden_size, num_heads=8):
        super().__init__()
        self.attention = nn.MultiheadAttention(embed_dim=hidden_size, num_heads=num_heads, batch_first=True)
        self.query = nn.Parameter(torch.randn(1, 1, hidden_size))

    def folded_query(self) -> torch.Tensor:
        """qt [heads, H] = hd^-0.5 W_k,h^T (W_q query + b_q)_h: score[h, l] = x_l . qt_h + const_h (b_k cancels in the softmax)"""
        att = self.attention
        H, nh = att.embed_dim, att.num_heads
        hd = H // nh
        q = att.in_proj_weight[:H] @ self.query.reshape(H) + att.in_proj_bias[:H]
        return torch.einsum("hd,hdk->hk", q.view(nh, hd), att.in_proj_weight[H:2 * H].view(nh, hd, H)) * hd ** -0.5

    def forward(self, embeddings, attention_mask=None):
        att = self.attention
        n, S, H = embeddings.shape
        nh = att.num_heads
        if attention_mask is None:
            mask = torch.ones((n, S), dtype=torch.uint8, device=embeddings.device)
        else:
            mask = (attention_mask != 0).to(device=embeddings.device, dtype=torch.uint8).contiguous()
        x = embeddings.detach()
        if x.dtype != BF16:
            x = x.to(BF16)
        if x.stride(2) != 1 or x.stride(1) % 8 or x.stride(0) % 8:
            x = x.contiguous()
        pooled = _AttnPoolFn.apply(x, mask, self.folded_query())                                   # [n, nh, H] fp32
        wv = att.in_proj_weight[2 * H:].view(nh, H // nh, H)
        ctx = torch.einsum("nhk,hdk->nhd", pooled, wv).reshape(n, H) + att.in_proj_bias[2 * H:]     # sum_l p = 1: b_v once
        return att.out_proj(ctx)


class DNAClassifierModel(nn.Module):
    """dna_only.py:42-203: frozen DNA encoder -> attention pooling of ref and alt -> MLP over [ref | alt]."""

    def __init__(
        self,
        dna_model_name: Union[str, Any],
        cache_dir: str = None,
        max_length_dna: int = 4096,
        num_classes: int = 2,
        dna_is_evo2: bool = False,
        dna_embedding_layer: str = None,
        train_just_classifier: bool = True,
        device: Optional[Union[str, torch.device]] = None,
    ):
        super().__init__()
        if not train_just_classifier:
            raise NotImplementedError("train_just_classifier=False fine-tunes the DNA encoder, and the HIP encoder engine has no "
                                      "backward pass; only the pooler and the classifier train here")
        self.dna_model_name, self.cache_dir, self.max_length_dna = dna_model_name, cache_dir, max_length_dna
        self.num_classes, self.dna_is_evo2, self.dna_embedding_layer = num_classes, dna_is_evo2, dna_embedding_layer
        self.train_just_classifier = train_just_classifier
        dev = torch.device(device) if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
        if dna_is_evo2:                                              # as DNALLMModel: a name needs `evo2`, an object is taken as it is
            from .evo2_tokenizer import Evo2Tokenizer
            if isinstance(dna_model_name, str):
                try:
                    from evo2 import Evo2
                except ImportError as e:
                    raise ImportError("dna_is_evo2=True with a checkpoint name needs the `evo2` package (not installed: SURVEY §8c); "
                                      "pass an encoder object with Evo2's call interface instead") from e
                self.dna_model = Evo2(dna_model_name)
            else:
                self.dna_model = dna_model_name
            self.dna_tokenizer = Evo2Tokenizer(getattr(self.dna_model, "tokenizer", None))
            self.dna_config = self.dna_model.model.config
            self.evo2_batched = bool(getattr(self.dna_model, "supports_batch", False))
        elif isinstance(dna_model_name, str):
            from .checkpoint import load_pretrained_dna
            self.dna_model, self.dna_tokenizer = load_pretrained_dna(dna_model_name, cache_dir, dev)
            self.dna_config = self.dna_model.config
        else:                                                        # a config object: random init (tests, offline)
            from .modeling import NTEncoderForMaskedLM
            self.dna_model, self.dna_tokenizer = NTEncoderForMaskedLM(dna_model_name, device=dev), None
            self.dna_config = self.dna_model.config
        if hasattr(self.dna_model, "parameters"):
            for p in self.dna_model.parameters():
                p.requires_grad_(False)
        self.hidden_size = self.dna_config.hidden_size
        self.pooler = SelfAttentionPooling(self.hidden_size)
        self.classifier = nn.Sequential(
            nn.Linear(self.hidden_size * 2, self.hidden_size),
            nn.ReLU(),
            nn.Dropout(0.1),
            nn.Linear(self.hidden_size, num_classes),
        )
        self.pooler.to(dev)
        self.classifier.to(dev)

    @torch.no_grad()
    def _hidden_states(self, input_ids: torch.Tensor, attention_mask: torch.Tensor) -> torch.Tensor:
        """frozen encoder over [n, S] token rows -> [n, S, H] bf16 (dna_only.py:133-155)"""
        if not (self.dna_is_evo2 and self.dna_embedding_layer is not None):
            return self.dna_model(input_ids=input_ids, attention_mask=attention_mask).hidden_states[-1]
        layer = self.dna_embedding_layer
        if self.evo2_batched:
            _, emb = self.dna_model(input_ids, return_embeddings=True, layer_names=[layer])
            h = emb[layer]
        else:                                                        # the reference's call per sequence
            rows = []
            for i in range(input_ids.shape[0]):
                _, emb = self.dna_model(input_ids[i:i + 1], return_embeddings=True, layer_names=[layer])
                rows.append(emb[layer].squeeze(0))
            h = torch.stack(rows)
        return h.to(device=self.pooler.query.device, dtype=BF16).contiguous()

    def get_dna_embedding(self, input_ids: torch.Tensor, attention_mask: torch.Tensor = None):
        """[S] or [n, S] token ids (+ mask) -> pooled embedding [H] or [n, H] (dna_only.py:111-159; `squeeze(0)` as there)"""
        if input_ids.dim() == 1:
            input_ids = input_ids.unsqueeze(0)
        if attention_mask is None:
            attention_mask = torch.ones_like(input_ids)
        elif attention_mask.dim() == 1:
            attention_mask = attention_mask.unsqueeze(0)
        hidden_states = self._hidden_states(input_ids, attention_mask)
        return self.pooler(hidden_states, attention_mask).squeeze(0)

    def forward(self, ref_ids=None, alt_ids=None, ref_attention_mask=None, alt_attention_mask=None):
        if ref_ids is None and alt_ids is None:
            raise ValueError("Either token IDs must be provided")
        B = ref_ids.shape[0]
        # one batched encoder call and one pooling per side (the reference: 2 B calls of one row, dna_only.py:185-191)
        ref = self.pooler(self._hidden_states(ref_ids, ref_attention_mask), ref_attention_mask).reshape(B, -1)
        alt = self.pooler(self._hidden_states(alt_ids, alt_attention_mask), alt_attention_mask).reshape(B, -1)
        return self.classifier(torch.cat([ref, alt], dim=1))
