"""Same export list as the reference's ``models`` package (models/__init__.py:1-14) for the
classes on the hot path and their scaffolding."""
from .attention import AgentAttention, SoftmaxAttention, SwitchHeadAttention
from .model_factory import build_model
from .moe import MoELayer
from .maskgit import BiDirectionalTransformer, MaskGitTransformer
from .muse import MUSE, BidirectionalDecoder
from .vit import ViT
from .vit_moe import ViTMoE
from .vitvqgan import Codebook, ViTVQGAN
from . import vqgan  # the conv VQGAN's own codebook stays vqgan.Codebook (models/vqgan.py:138-182)
from .vqgan import VQGAN

__all__ = ["SoftmaxAttention", "AgentAttention", "SwitchHeadAttention", "MoELayer", "Codebook", "ViTVQGAN", "VQGAN",
           "ViT", "ViTMoE", "MUSE", "BidirectionalDecoder", "MaskGitTransformer", "BiDirectionalTransformer", "build_model"]
