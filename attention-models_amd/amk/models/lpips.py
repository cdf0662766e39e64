"""LPIPS(vgg), the perceptual term of the reference's generator loss (trainers/vitgqgan.py:173-181,
``per_loss_weight`` of cfg/vitvqgan.yaml:67), written from the published definition of lpips 0.1.4,
``LPIPS(net='vgg', version='0.1', lpips=True, spatial=False)``: a scaling layer, torchvision's ``vgg16().features[0:30]``
cut at the ReLUs 3, 8, 15, 22 and 29, and per level a distance head (unit-normalise both feature tensors over the channels,
weight the squared difference with a 1x1 convolution, average over the pixels).  The value is the sum of the five heads,
(N, 1, 1, 1).

What differs from the package, and why.  The package downloads the VGG weights and ships the lin weights; neither is
available here, so the module is built with whatever the random generator gives (``torch.manual_seed`` first for
reproducible ones; the lin weights are made non-negative, as the trained ones are) and takes the weights a user already
has: ``model_path`` for a lin-weight file of the package (``weights/v0.1/vgg.pth``: its keys ``lin*.model.1.weight`` are
this module's) and ``load_vgg16_features`` for torchvision's ``vgg16`` state_dict.  The module tree reproduces the
package's state_dict keys, so a whole LPIPS state_dict loads too.  ``pretrained=True`` without a ``model_path`` raises.
Every parameter is frozen in the constructor, the lin weights included (the package leaves those trainable; training them
is not built here): a caller who sets ``requires_grad`` on a lin weight gets the torch chain for that level.

The convolutions run on the vendor library.  The heads go through ``ops.lpips_distance``: with ``AMK_LPIPS=1`` (it ships
off: the step with the term is not measured yet) csrc/lpips.hip's fused forward and gradient for ``in0``'s features when those are contiguous f32 HIP tensors (bf16 under bf16 autocast), the
lin weights and ``in1`` need no gradient and the module is not applying dropout; the torch chain of the package otherwise.
Two differences of the fused path, both deliberate: under bf16 autocast it returns f32 where the chain returns bf16 (the
sums are taken in f32 either way it is called from here on); and a pixel whose ``in0`` features are all zero gets a zero
gradient where autograd computes NaN (sqrt'(0) * 0) -- the in-place ReLU in front of every level discards what arrives at
such a pixel, so the gradient that leaves the tower is the same and finite.  ``in1`` runs through the tower under
``no_grad`` when nothing behind it needs a gradient, so its activations are not kept.
"""
import torch
import torch.nn as nn

from .. import ops

# torchvision's vgg16().features[0:30]: index -> (in, out) of the 3x3 convolutions; ReLU after each; 2x2 max pools at POOLS
_CONVS = {0: (3, 64), 2: (64, 64), 5: (64, 128), 7: (128, 128), 10: (128, 256), 12: (256, 256), 14: (256, 256),
          17: (256, 512), 19: (512, 512), 21: (512, 512), 24: (512, 512), 26: (512, 512), 28: (512, 512)}
_POOLS = (4, 9, 16, 23)
_SLICES = ((0, 4), (4, 9), (9, 16), (16, 23), (23, 30))
CHANNELS = (64, 128, 256, 512, 512)
EPS = 1e-10


class ScalingLayer(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.tensor([-.030, -.088, -.188])[None, :, None, None])
        self.register_buffer("scale", torch.tensor([.458, .448, .450])[None, :, None, None])

    def forward(self, x):
        return (x - self.shift) / self.scale


class VGG16Features(nn.Module):
    """slice1 .. slice5, each module under torchvision's index as its name; returns the five ReLU outputs."""

    def __init__(self):
        super().__init__()
        for k, (lo, hi) in enumerate(_SLICES):
            seq = nn.Sequential()
            for i in range(lo, hi):
                if i in _CONVS:
                    seq.add_module(str(i), nn.Conv2d(*_CONVS[i], kernel_size=3, padding=1))
                elif i in _POOLS:
                    seq.add_module(str(i), nn.MaxPool2d(kernel_size=2, stride=2))
                else:
                    seq.add_module(str(i), nn.ReLU(inplace=True))
            setattr(self, f"slice{k + 1}", seq)

    def forward(self, x):
        outs = []
        for k in range(5):
            x = getattr(self, f"slice{k + 1}")(x)
            outs.append(x)
        return outs


class NetLinLayer(nn.Module):
    """The package's 1x1 convolution without bias, behind a Dropout when use_dropout (so the weight is model.1.weight)."""

    def __init__(self, chn_in, chn_out=1, use_dropout=False):
        super().__init__()
        layers = [nn.Dropout()] if use_dropout else []
        layers += [nn.Conv2d(chn_in, chn_out, 1, stride=1, padding=0, bias=False)]
        self.model = nn.Sequential(*layers)
        self.use_dropout = bool(use_dropout)
        with torch.no_grad():
            self.model[-1].weight.abs_()

    def forward(self, x):
        return self.model(x)


def normalize_tensor(x, eps=EPS):
    return x / (torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True)) + eps)


class LPIPS(nn.Module):
    def __init__(self, net="vgg", pretrained=False, model_path=None, use_dropout=True, spatial=False, eval_mode=True):
        super().__init__()
        if net != "vgg":
            raise NotImplementedError(f"LPIPS(net={net!r}): only the vgg tower is built here")
        if spatial:
            raise NotImplementedError("LPIPS(spatial=True): only the spatially averaged value is built here")
        if pretrained and model_path is None:
            raise RuntimeError("LPIPS(pretrained=True) needs the lpips package's lin weights (weights/v0.1/vgg.pth) and "
                               "torchvision's vgg16 weights, a download that is not available: pass model_path for the "
                               "former and call load_vgg16_features(state_dict) with the latter")
        self.scaling_layer = ScalingLayer()
        self.net = VGG16Features()
        for k, c in enumerate(CHANNELS):
            setattr(self, f"lin{k}", NetLinLayer(c, use_dropout=use_dropout))
        self.lins = nn.ModuleList([getattr(self, f"lin{k}") for k in range(5)])
        # a fixed metric: the tower as in the package (pnet_tune=False), and the lin weights too -- training them is not built,
        # and a lin weight that requires grad would send its head to the torch chain (ops.lpips_distance_ok)
        self.requires_grad_(False)
        if model_path is not None:
            self.load_state_dict(torch.load(model_path, map_location="cpu", weights_only=True), strict=False)
        if eval_mode:
            self.eval()

    def load_vgg16_features(self, state_dict):
        """Copy torchvision's vgg16 convolutions in: keys ``features.N.weight`` / ``.bias`` or ``N.weight`` / ``.bias``
        for the thirteen N below 30; other keys (the classifier) are ignored."""
        mapped = {}
        for k, (lo, hi) in enumerate(_SLICES):
            for i in range(lo, hi):
                if i not in _CONVS:
                    continue
                for leaf in ("weight", "bias"):
                    src = next((key for key in (f"features.{i}.{leaf}", f"{i}.{leaf}") if key in state_dict), None)
                    if src is None:
                        raise KeyError(f"load_vgg16_features: neither features.{i}.{leaf} nor {i}.{leaf} in the state_dict")
                    mapped[f"slice{k + 1}.{i}.{leaf}"] = state_dict[src]
        self.net.load_state_dict(mapped, strict=True)
        return self

    def _head(self, k, a, b):
        lin = self.lins[k]
        if self.training and lin.use_dropout:
            d = (normalize_tensor(a) - normalize_tensor(b)) ** 2
            return lin(d).mean([2, 3], keepdim=True)
        return ops.lpips_distance(a, b, lin.model[-1].weight.reshape(-1), EPS).reshape(-1, 1, 1, 1)

    def forward(self, in0, in1, retPerLayer=False, normalize=False):
        if normalize:
            in0, in1 = 2 * in0 - 1, 2 * in1 - 1
        outs0 = self.net(self.scaling_layer(in0))
        if in1.requires_grad or any(p.requires_grad for p in self.net.parameters()):
            outs1 = self.net(self.scaling_layer(in1))
        else:
            with torch.no_grad():
                outs1 = self.net(self.scaling_layer(in1))
        res = [self._head(k, outs0[k], outs1[k]) for k in range(5)]
        val = res[0]
        for r in res[1:]:
            val = val + r
        return (val, res) if retPerLayer else val
