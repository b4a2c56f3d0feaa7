"""The encoders `--backbone` may name (the reference resolves any constructor of models/vit/vit.py by name, models/__init__.py:87).

Built: ViT-B/16 (`vit_base_patch16_224`, models/vit/vit.py:365-377) and the self-supervised DINO ViT-B/8 (`dino_base_patch8_224`,
models/vit/vit.py:355-363).  Both have ViT-B's width, heads, depth, MLP ratio, qkv bias and LayerNorm eps, so every kernel that assumes
width 768 holds for both; the 8-pixel patch changes the token geometry only (K = 3*8*8 = 192 patch columns, 4x the tokens, CAMs at S/8).
"""
import os

from .vit import VisionTransformer, load_pretrained_vit, vit_base_patch16_224

DINO_B8_PRETRAINED_ENV = "COSA_DINO_B8_PRETRAINED"     # path of a local DINO ViT-B/8 checkpoint (dino_vitbase8_pretrain.pth)


def dino_base_patch8_224(pretrained=False, pretrained_path=None, **kwargs):
    """models/vit/vit.py:355-363.  The weights come from a local file (`pretrained_path`, or $COSA_DINO_B8_PRETRAINED -- never the ViT-B/16
    variable): DINO's checkpoint is a plain state dict with timm key names and no `head.*`.  pretrained=True without a file fails."""
    model = VisionTransformer(img_size=224, patch_size=8, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4, qkv_bias=True, eps=1e-6,
                              **kwargs)
    if pretrained:
        path = pretrained_path or os.environ.get(DINO_B8_PRETRAINED_ENV)
        if not path or not os.path.exists(path):
            raise FileNotFoundError(
                "dino_base_patch8_224(pretrained=True): no local checkpoint -- pass pretrained_path= or set $" + DINO_B8_PRETRAINED_ENV +
                " to the DINO ViT-B/8 backbone weights (dino_vitbase8_pretrain.pth), or build with pretrained=False")
        load_pretrained_vit(model, path)
    return model


BACKBONES = {
    "vit_base_patch16_224": vit_base_patch16_224,
    "dino_base_patch8_224": dino_base_patch8_224,
}


def get_backbone(name):
    """the constructor of encoder `name`; NotImplementedError naming the built ones for any other"""
    ctor = BACKBONES.get(name)
    if ctor is None:
        raise NotImplementedError(f"--backbone {name}: not built; the built backbones are {', '.join(sorted(BACKBONES))}")
    return ctor
