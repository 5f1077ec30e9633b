"""bioreason/models/dna_only.py:8-203 -> bioreason_amd.dna_only"""
from bioreason_amd.dna_only import DNAClassifierModel, SelfAttentionPooling  # noqa: F401
