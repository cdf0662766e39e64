"""Position signals of the autoregressive models (reference: models/positional_encoding.py:9-42).  Plain PyTorch: one
add per forward."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F


class AbsolutePositionalEmbedding(nn.Module):
    """A learned table of max_len positions, L2-normalised per position (reference :9-18)."""

    def __init__(self, dim, max_len):
        super().__init__()
        self.emb = nn.Embedding(max_len, dim)

    def forward(self, x):
        return F.normalize(self.emb(x), p=2, dim=-1)


class PositionalEncoding(nn.Module):
    """x + pe[:seq_len], then dropout (reference :22-42).  ``pe`` is a BUFFER of (max_len, dim), sines in the even
    columns and cosines in the odd ones: it is in the state_dict, as in the reference."""

    def __init__(self, dim, dropout=0.1, max_len=5000):
        super().__init__()
        self.dropout = nn.Dropout(p=dropout)
        position = torch.arange(max_len).unsqueeze(1)
        div_term = torch.exp(torch.arange(0, dim, 2) * (-math.log(10000.0) / dim))
        pe = torch.zeros(max_len, dim)
        pe[:, 0::2] = torch.sin(position * div_term)
        pe[:, 1::2] = torch.cos(position * div_term)
        self.register_buffer("pe", pe)

    def forward(self, x):
        """x: (batch, seq_len, dim)."""
        return self.dropout(x + self.pe[: x.size(1)])
