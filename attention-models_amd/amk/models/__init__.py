"""The export list of the reference's ``models`` package (models/__init__.py:1-14), all fourteen names, and the
scaffolding around them."""
from .attention import AgentAttention, SoftmaxAttention, SwitchHeadAttention
from .model_factory import build_model
from .moe import MoELayer
from .maskgit import BiDirectionalTransformer, MaskGitTransformer
from .muse import MUSE, BidirectionalDecoder
from .parti import Parti
from .positional_encoding import AbsolutePositionalEmbedding, PositionalEncoding
from .transformer import Transformer
from .vit import ViT
from .vit_moe import ViTMoE
from .vitvqgan import Codebook, ViTVQGAN
from . import vqgan  # the conv VQGAN's own codebook stays vqgan.Codebook (models/vqgan.py:138-182)
from .vqgan import VQGAN
from .lpips import LPIPS  # the GAN step's perceptual loss: not a name of the reference's package, so not in __all__ (the alias package re-exports that)

__all__ = ["SoftmaxAttention", "AgentAttention", "SwitchHeadAttention", "MoELayer", "Codebook", "ViTVQGAN", "VQGAN",
           "ViT", "ViTMoE", "MUSE", "BidirectionalDecoder", "MaskGitTransformer", "BiDirectionalTransformer", "build_model",
           "Parti", "Transformer", "PositionalEncoding", "AbsolutePositionalEmbedding"]
