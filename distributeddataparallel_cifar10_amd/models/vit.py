"""Vision transformer (Dosovitskiy et al. 2021, "An Image is Worth 16x16 Words"): patch embedding as a strided conv, a
class token and a learned position embedding, ``depth`` pre-LayerNorm blocks (LN -> qkv Linear -> multi-head
self-attention -> proj Linear -> add; LN -> Linear -> GELU -> Linear -> add), a final LN and a Linear head on the class
token.  No dropout.  The qkv Linear's output is split as [B, L, 3, heads, D]: the layout csrc/ops_attn.hip reads.

On the ops path (``OpsModel``) every Linear runs on the MFMA GEMMs, the attention on csrc/ops_attn.hip, and the
LayerNorms (each fused with the residual add before it) and the GELU on csrc/ops_ln.hip; this
module's own forward is stock torch (``scaled_dot_product_attention``) and runs on the CPU.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as TF


class Block(nn.Module):
    def __init__(self, dim: int, heads: int, mlp_ratio: float):
        super().__init__()
        self.heads = heads
        self.norm1 = nn.LayerNorm(dim)
        self.qkv = nn.Linear(dim, 3 * dim)
        self.proj = nn.Linear(dim, dim)
        self.norm2 = nn.LayerNorm(dim)
        self.fc1 = nn.Linear(dim, int(dim * mlp_ratio))
        self.fc2 = nn.Linear(int(dim * mlp_ratio), dim)

    def attention(self, x: torch.Tensor) -> torch.Tensor:
        b, l, dim = x.shape
        q, k, v = self.qkv(x).view(b, l, 3, self.heads, dim // self.heads).permute(2, 0, 3, 1, 4)  # each [B, H, L, D]
        return TF.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(b, l, dim)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = x + self.proj(self.attention(self.norm1(x)))
        return x + self.fc2(TF.gelu(self.fc1(self.norm2(x))))


class VisionTransformer(nn.Module):
    def __init__(self, img_size: int = 224, patch: int = 16, dim: int = 192, depth: int = 12, heads: int = 3,
                 mlp_ratio: float = 4, num_classes: int = 1000):
        super().__init__()
        if img_size % patch or dim % heads:
            raise ValueError(f"VisionTransformer: img_size {img_size} % patch {patch} and dim {dim} % heads {heads} "
                             "must be 0")
        self.patch, self.dim, self.heads = patch, dim, heads
        self.patch_embed = nn.Conv2d(3, dim, patch, stride=patch)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, (img_size // patch) ** 2 + 1, dim))
        nn.init.trunc_normal_(self.cls_token, std=0.02)
        nn.init.trunc_normal_(self.pos_embed, std=0.02)
        self.blocks = nn.Sequential(*[Block(dim, heads, mlp_ratio) for _ in range(depth)])
        self.norm = nn.LayerNorm(dim)
        self.head = nn.Linear(dim, num_classes)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = self.patch_embed(x).flatten(2).transpose(1, 2)  # [B, L - 1, dim]
        x = torch.cat([self.cls_token.expand(x.shape[0], -1, -1), x], dim=1) + self.pos_embed
        return self.head(self.norm(self.blocks(x))[:, 0])


def vit_tiny(num_classes: int = 1000, img_size: int = 32, patch: int = 4) -> VisionTransformer:
    """ViT-Tiny: dim 192, 3 heads of 64, depth 12; 65 tokens on the CIFAR tensors, 197 at 224 / 16."""
    return VisionTransformer(img_size, patch, dim=192, depth=12, heads=3, mlp_ratio=4, num_classes=num_classes)
