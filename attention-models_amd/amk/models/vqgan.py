"""Conv VQGAN (taming-style) on the libamk.so VQ and GroupNorm + Swish kernels.

Reference: models/vqgan.py.  The module tree reproduces the reference's state_dict keys (``encoder.model.1.block.0.gn.weight``,
``encoder.model.14.q.weight``, ``decoder.model.0.weight`` ...), so a reference checkpoint loads with ``strict=True``.

Convolutions stay on the vendor library.  Every ``GroupNorm(32, C, eps=1e-6)`` -> ``Swish`` pair, about 60 per forward, runs
as one fused op, ``ops.group_norm_act(x, gn, 1)`` (csrc/gn_act.hip), which recomputes the normalised tensor in the backward
instead of storing it; the ``gn`` inside ``NonLocalBlock`` runs the same kernels without the activation.  Containers that
hold a ``GroupNorm`` followed by a ``Swish`` (``ResidualBlock.block``, the tails of ``Encoder.model`` / ``Decoder.model``) are
walked by ``_run``, which fuses each such pair and calls every other layer as it is; ``Swish`` therefore has no parameters and
is skipped after a fused pair.  With ``AMK_GN_ACT=0``, on the CPU or for a non-contiguous input the op keeps the modules
(``nn.GroupNorm`` and ``x * sigmoid(x)``).

Under ``torch.autocast("cuda", dtype=torch.bfloat16)`` every norm sits behind a convolution (or behind ``F.pad`` /
``F.interpolate`` / a residual sum of convolution outputs), so its input is a contiguous bf16 tensor, and all 70 run on the
bf16 form of the same kernels (``amk_gnact_bf16_*``, ``AMK_GN_ACT_BF16``): bf16 in, f32 arithmetic, bf16 out rounded once,
where the modules would cast to f32, run three f32 passes and leave the rounding to the next convolution.  ``encode_imgs`` /
``decode_indices`` under autocast and ``no_grad`` (a frozen tokenizer) take the forward kernel and save nothing.

Codebook (models/vqgan.py:138-182): the same l2-normalised nearest-neighbour lookup as the ViT-VQGAN codebook with a
channels-first ``(B, C, H, W)`` input, ``codebook_dim`` 256 by default (README.md:246-249), uniform init, ``beta`` on the
codebook term instead of the commitment term, flat ``(B*H*W,)`` indices and an ``indices_to_embeddings`` that returns the raw
rows.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops


class GroupNorm(nn.Module):
    def __init__(self, channels):
        super().__init__()
        self.gn = nn.GroupNorm(num_groups=32, num_channels=channels, eps=1e-6, affine=True)

    def forward(self, x, act=0):
        return ops.group_norm_act(x, self.gn, act)


class Swish(nn.Module):
    def forward(self, x):
        return x * torch.sigmoid(x)


def _run(layers, x):
    """x through the layers of an nn.Sequential, each GroupNorm -> Swish pair as one fused call."""
    layers = list(layers)
    i = 0
    while i < len(layers):
        m = layers[i]
        if isinstance(m, GroupNorm) and i + 1 < len(layers) and isinstance(layers[i + 1], Swish):
            x = m(x, act=1)
            i += 2
        else:
            x = m(x)
            i += 1
    return x


class ResidualBlock(nn.Module):
    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.block = nn.Sequential(
            GroupNorm(in_channels), Swish(), nn.Conv2d(in_channels, out_channels, 3, 1, 1),
            GroupNorm(out_channels), Swish(), nn.Conv2d(out_channels, out_channels, 3, 1, 1))
        if in_channels != out_channels:
            self.channel_up = nn.Conv2d(in_channels, out_channels, 1, 1, 0)

    def forward(self, x):
        skip = self.channel_up(x) if self.in_channels != self.out_channels else x
        return skip + _run(self.block, x)


class UpSampleBlock(nn.Module):
    def __init__(self, channels):
        super().__init__()
        self.conv = nn.Conv2d(channels, channels, 3, 1, 1)

    def forward(self, x):
        return self.conv(F.interpolate(x, scale_factor=2.0))      # nearest


class DownSampleBlock(nn.Module):
    def __init__(self, channels):
        super().__init__()
        self.conv = nn.Conv2d(channels, channels, 3, 2, 0)

    def forward(self, x):
        return self.conv(F.pad(x, (0, 1, 0, 1), mode="constant", value=0))   # right and bottom by one


class NonLocalBlock(nn.Module):
    """Single-head self-attention over the h w positions of a feature map, width = channels (512 in this model).

    The head dim 512 is outside the attention kernels' head dims, which stop at 256; at the 256 tokens of the 16 x 16 maps
    it is a negligible share of the model's work and stays on library bmm + softmax.  ``proj_out`` is never applied, as in
    the reference (models/vqgan.py:79-102): its parameters exist for the state_dict and get no gradient."""

    def __init__(self, channels):
        super().__init__()
        self.in_channels = channels
        self.gn = GroupNorm(channels)
        self.q = nn.Conv2d(channels, channels, 1, 1, 0)
        self.k = nn.Conv2d(channels, channels, 1, 1, 0)
        self.v = nn.Conv2d(channels, channels, 1, 1, 0)
        self.proj_out = nn.Conv2d(channels, channels, 1, 1, 0)

    def forward(self, x):
        h_ = self.gn(x, act=0)
        b, c, h, w = x.shape
        q = self.q(h_).reshape(b, c, h * w).permute(0, 2, 1)
        k = self.k(h_).reshape(b, c, h * w)
        v = self.v(h_).reshape(b, c, h * w)
        attn = F.softmax(torch.bmm(q, k) * (int(c) ** (-0.5)), dim=2)
        return x + torch.bmm(v, attn.permute(0, 2, 1)).reshape(b, c, h, w)


class Encoder(nn.Module):
    def __init__(self, dim):
        super().__init__()
        channels = [128, 128, 128, 256, 256, 512]
        resolution, attn_resolutions, num_res_blocks = 256, (16,), 2
        layers = [nn.Conv2d(3, channels[0], 3, 1, 1)]
        for i in range(len(channels) - 1):
            cin, cout = channels[i], channels[i + 1]
            for _ in range(num_res_blocks):
                layers.append(ResidualBlock(cin, cout))
                cin = cout
                if resolution in attn_resolutions:
                    layers.append(NonLocalBlock(cin))
            if i != len(channels) - 2:
                layers.append(DownSampleBlock(cout))
                resolution //= 2
        layers += [ResidualBlock(channels[-1], channels[-1]), NonLocalBlock(channels[-1]),
                   ResidualBlock(channels[-1], channels[-1]), GroupNorm(channels[-1]), Swish(),
                   nn.Conv2d(channels[-1], dim, 3, 1, 1)]
        self.num_patches = 16 * 16          # a constant in the reference too, whatever the input size
        self.model = nn.Sequential(*layers)

    def forward(self, x):
        return _run(self.model, x)


class Codebook(nn.Module):
    def __init__(self, codebook_size=1024, codebook_dim=256, beta=0.25):
        super().__init__()
        self.codebook_size = codebook_size
        self.codebook_dim = codebook_dim
        self.beta = beta
        self.embedding = nn.Embedding(codebook_size, codebook_dim)
        self.embedding.weight.data.uniform_(-1.0 / codebook_size, 1.0 / codebook_size)

    def forward(self, z):
        zt = z.permute(0, 2, 3, 1)                                  # 'b d h w -> b h w d'
        # the kernel's loss is  w * mean((zq.detach() - z)^2) + mean((zq - z.detach())^2); the reference's
        # weights here are (1, beta) = beta * (1/beta, 1)
        z_q, idx, loss = ops.vq_lookup(zt, self.embedding.weight, 1.0 / self.beta)
        return z_q.permute(0, 3, 1, 2), idx.reshape(-1), self.beta * loss

    def indices_to_embeddings(self, indices):
        e = self.embedding(indices)                                  # (B, T, C), no l2-norm here
        side = int(e.shape[1] ** 0.5)
        return e.view(e.shape[0], side, side, -1).permute(0, 3, 1, 2)


class Decoder(nn.Module):
    def __init__(self, dim):
        super().__init__()
        channels = [512, 256, 256, 128, 128]
        resolution, attn_resolutions, num_res_blocks = 16, (16,), 3
        cin = channels[0]
        layers = [nn.Conv2d(dim, cin, 3, 1, 1), ResidualBlock(cin, cin), NonLocalBlock(cin), ResidualBlock(cin, cin)]
        for i, cout in enumerate(channels):
            for _ in range(num_res_blocks):
                layers.append(ResidualBlock(cin, cout))
                cin = cout
                if resolution in attn_resolutions:
                    layers.append(NonLocalBlock(cin))
            if i != 0:
                layers.append(UpSampleBlock(cin))
                resolution *= 2
        layers += [GroupNorm(cin), Swish(), nn.Conv2d(cin, 3, 3, 1, 1)]
        self.model = nn.Sequential(*layers)

    def forward(self, x):
        return _run(self.model, x)


class VQGAN(nn.Module):
    """``VQGAN(dim, codebook_size)``: conv encoder (256 px -> 16 x 16 x dim), codebook, conv decoder."""

    def __init__(self, dim, codebook_size):
        super().__init__()
        self.encoder = Encoder(dim)
        self.pre_quant = nn.Conv2d(dim, dim, 1)
        self.codebook = Codebook(codebook_size, dim)
        self.post_quant = nn.Conv2d(dim, dim, 1)
        self.decoder = Decoder(dim)

    def forward(self, imgs):
        embeds, _, loss = self.codebook(self.pre_quant(self.encoder(imgs)))
        # the codebook hands back a permuted (channels-last) view, and convolutions keep their input's layout: made
        # contiguous here (dim x 16 x 16 floats), the whole decoder runs in NCHW and its GroupNorms take the fused kernels
        return self.decoder(self.post_quant(embeds.contiguous())), loss

    def decode_indices(self, indices):
        return self.decoder(self.post_quant(self.codebook.indices_to_embeddings(indices).contiguous()))

    def encode_imgs(self, imgs):
        _, indices, _ = self.codebook(self.pre_quant(self.encoder(imgs)))
        return indices.view(imgs.shape[0], -1)                      # (B, h w) int64

    @property
    def num_patches(self):
        return self.encoder.num_patches
