"""Stand-in for ``torchvision.models.vit_b_16`` composed of ``torch.nn`` modules (torchvision is not installed where the
fixtures are generated).  Written from torchvision's published ``VisionTransformer`` module layout: same attribute names, same
``state_dict`` keys and shapes, same arithmetic (Conv2d patch embedding, LayerNorm eps 1e-6, nn.MultiheadAttention with
batch_first, Linear-GELU-Linear MLP).  It is the CPU reference of the ViT-B/16 trunk tests, and
``tests/golden/make_golden_vit.py`` installs it as ``torchvision.models.vit_b_16`` so that the real reference model constructs.
``tests/test_vit_backbone.py`` checks its encoder against the independent ``transformers.ViTModel``."""
from collections import OrderedDict

import torch
import torch.nn as nn


class MLPBlock(nn.Sequential):
    def __init__(self, dim, mlp_dim):
        super().__init__(nn.Linear(dim, mlp_dim), nn.GELU(), nn.Dropout(0.0), nn.Linear(mlp_dim, dim), nn.Dropout(0.0))


class EncoderBlock(nn.Module):
    def __init__(self, heads, dim, mlp_dim):
        super().__init__()
        self.ln_1 = nn.LayerNorm(dim, eps=1e-6)
        self.self_attention = nn.MultiheadAttention(dim, heads, dropout=0.0, batch_first=True)
        self.dropout = nn.Dropout(0.0)
        self.ln_2 = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = MLPBlock(dim, mlp_dim)

    def forward(self, x):
        y = self.ln_1(x)
        y, _ = self.self_attention(y, y, y, need_weights=False)
        x = x + self.dropout(y)
        return x + self.mlp(self.ln_2(x))


class Encoder(nn.Module):
    def __init__(self, seq_length, layers, heads, dim, mlp_dim):
        super().__init__()
        self.pos_embedding = nn.Parameter(torch.empty(1, seq_length, dim).normal_(std=0.02))
        self.dropout = nn.Dropout(0.0)
        self.layers = nn.Sequential(OrderedDict((f"encoder_layer_{i}", EncoderBlock(heads, dim, mlp_dim)) for i in range(layers)))
        self.ln = nn.LayerNorm(dim, eps=1e-6)

    def forward(self, x):
        return self.ln(self.layers(self.dropout(x + self.pos_embedding)))


class VisionTransformer(nn.Module):
    def __init__(self, image_size=224, patch_size=16, num_layers=12, num_heads=12, hidden_dim=768, mlp_dim=3072, num_classes=1000):
        super().__init__()
        self.image_size, self.patch_size, self.hidden_dim = image_size, patch_size, hidden_dim
        self.conv_proj = nn.Conv2d(3, hidden_dim, kernel_size=patch_size, stride=patch_size)
        self.class_token = nn.Parameter(torch.zeros(1, 1, hidden_dim))
        self.encoder = Encoder((image_size // patch_size) ** 2 + 1, num_layers, num_heads, hidden_dim, mlp_dim)
        self.heads = nn.Sequential(OrderedDict(head=nn.Linear(hidden_dim, num_classes)))

    def _process_input(self, x):
        n, _, h, w = x.shape
        p = self.patch_size
        x = self.conv_proj(x)                                  # (n, hidden, h / p, w / p)
        return x.reshape(n, self.hidden_dim, (h // p) * (w // p)).permute(0, 2, 1)

    def forward(self, x):
        x = self._process_input(x)
        x = torch.cat([self.class_token.expand(x.shape[0], -1, -1), x], dim=1)
        return self.heads(self.encoder(x)[:, 0])


def vit_b_16(weights=None, **kw):
    """No weights are fetched: ``weights`` is accepted (the reference passes 'DEFAULT') and ignored."""
    return VisionTransformer()


def vit_conv():
    """src/nets/backbone/utils.py:27-34 restated for the trunk tests (the fixtures run the reference's own)."""
    return nn.Sequential(nn.AvgPool2d(kernel_size=2, stride=2), nn.Conv2d(768, 2048, kernel_size=3, stride=1, padding=1),
                         nn.BatchNorm2d(2048), nn.ReLU(inplace=True))


def vit_trunk_features(net, net_conv, images):
    """``HandsLight.vit_forward`` (model.py:483-493): images (B,C,224,224) -> (B,2048,7,7)."""
    conv_feat = net._process_input(images)
    bz = conv_feat.shape[0]
    x = torch.cat([net.class_token.expand(bz, -1, -1), conv_feat], dim=1)
    x = net.encoder(x)
    g = net.image_size // net.patch_size
    spatial = x[:, 1:].permute(0, 2, 1).reshape(bz, -1, g, g)
    return net_conv(spatial)
