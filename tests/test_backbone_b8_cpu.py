"""The DINO ViT-B/8 encoder (`--backbone dino_base_patch8_224`, reference models/vit/vit.py:355-363) on the host: launcher, constructor, weight
loading, and the refusal of the teacher modes it is not built for."""
import pytest
import torch


def _args(*extra):
    from cosa_amd import args as cosa_args
    return cosa_args.parse(["exp", "--pretrained", "false"] + list(extra))[0]


def test_launcher_parses_and_accepts_the_b8_backbone():
    from cosa_amd.main import check_supported
    a = _args("--backbone", "dino_base_patch8_224")
    assert a.backbone == "dino_base_patch8_224"
    check_supported(a)


def test_unknown_backbone_is_refused_with_the_built_list():
    from cosa_amd.main import check_supported
    from cosa_amd.models import VITNetwork
    with pytest.raises(NotImplementedError, match="dino_base_patch8_224.*vit_base_patch16_224"):
        check_supported(_args("--backbone", "vit_large_patch16_224"))
    with pytest.raises(NotImplementedError, match="vit_small_patch16_224"):
        VITNetwork("vit_small_patch16_224", 21, pretrained=False)


def _net(backbone):
    from cosa_amd.main import _trainer_args
    from cosa_amd.models import build_model
    return build_model(_trainer_args(_args("--backbone", backbone)))


def test_build_model_has_the_reference_keys_and_shapes():
    torch.manual_seed(0)
    b8, b16 = _net("dino_base_patch8_224").state_dict(), _net("vit_base_patch16_224").state_dict()
    assert list(b8) == list(b16)                               # the same module tree: ViT-B width / depth / heads, LargeFOV, two CAM heads
    assert tuple(b8["encoder.patch_embed.proj.weight"].shape) == (768, 3, 8, 8)
    assert tuple(b8["encoder.pos_embed"].shape) == (1, 785, 768)
    assert all(b8[k].shape == b16[k].shape for k in b8 if k not in ("encoder.patch_embed.proj.weight", "encoder.pos_embed"))
    enc = _net("dino_base_patch8_224").encoder
    assert enc.patch_size == 8 and len(enc.blocks) == 12 and enc.num_heads == 12 and enc.norm.eps == 1e-6
    assert enc.blocks[0].attn.qkv.bias is not None and enc.blocks[0].mlp.fc1.weight.shape == (3072, 768)


def test_dino_format_checkpoint_loads_strictly(tmp_path, monkeypatch):
    from cosa_amd.models.backbones import DINO_B8_PRETRAINED_ENV, dino_base_patch8_224
    torch.manual_seed(1)
    src = dino_base_patch8_224()
    sd = {k: v.clone() for k, v in src.state_dict().items() if not k.startswith("head.")}      # DINO: timm names, no classifier head
    sd["patch_embed.proj.weight"] = sd["patch_embed.proj.weight"].reshape(768, -1)           # (a linear-shaped projection is accepted too)
    path = tmp_path / "dino_vitbase8_pretrain.pth"
    torch.save(sd, path)
    monkeypatch.setenv(DINO_B8_PRETRAINED_ENV, str(path))
    m = dino_base_patch8_224(pretrained=True)
    own = m.state_dict()
    for k, v in src.state_dict().items():
        if not k.startswith("head."):
            assert torch.equal(own[k], v), k
    sd["blocks.0.attn.qkv.weight_extra"] = torch.zeros(1)
    torch.save(sd, path)
    with pytest.raises(RuntimeError, match="unexpected"):
        dino_base_patch8_224(pretrained=True)


def test_missing_checkpoint_names_its_own_variable_and_never_the_b16_one(tmp_path, monkeypatch):
    from cosa_amd.models import vit
    from cosa_amd.models.backbones import DINO_B8_PRETRAINED_ENV, dino_base_patch8_224
    b16 = tmp_path / "b16.pth"
    torch.save(vit.vit_base_patch16_224().state_dict(), b16)
    monkeypatch.setenv(vit.PRETRAINED_ENV, str(b16))                     # a ViT-B/16 file must not be picked up
    monkeypatch.delenv(DINO_B8_PRETRAINED_ENV, raising=False)
    with pytest.raises(FileNotFoundError, match=DINO_B8_PRETRAINED_ENV):
        dino_base_patch8_224(pretrained=True)
    from cosa_amd.models import VITNetwork
    with pytest.raises(FileNotFoundError, match=DINO_B8_PRETRAINED_ENV):
        VITNetwork("dino_base_patch8_224", 21, pretrained=True)


@pytest.mark.parametrize("mode", ["fp16c8", "fp16c8-x2", "fp16c8-9", "fp16c4", "fp16c4-9m7"])
def test_c8_and_c4_teacher_modes_are_refused_at_set_up_for_patch_8(mode):
    net = _net("dino_base_patch8_224")
    with pytest.raises(NotImplementedError, match="dino_base_patch8_224"):
        net.set_nograd_precision(mode)
    _net("vit_base_patch16_224").set_nograd_precision(mode)                  # ViT-B/16 keeps them


@pytest.mark.parametrize("mode", ["fp16x3", "bf16x3", "bf16", "fp16"])
def test_the_built_teacher_modes_are_accepted_for_patch_8(mode):
    _net("dino_base_patch8_224").set_nograd_precision(mode)


def test_trainer_refuses_a_c8_teacher_for_patch_8_before_any_step():
    from cosa_amd.main import _trainer_args
    from cosa_amd.train_step import CoSATrainer
    a = _trainer_args(_args("--backbone", "dino_base_patch8_224", "--teacher_precision", "fp16c8-x2", "--crop_size", "64"))
    a.compute_dtype = torch.bfloat16
    with pytest.raises(NotImplementedError, match="fp16c8-x2"):
        CoSATrainer(a, torch.device("cpu"))
