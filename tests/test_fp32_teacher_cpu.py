"""The "fp32" operand mode of the no-grad passes without a GPU: the mode string, the operand map, the empty weight
sets, the flags, and that the defaults did not move."""
import pytest
import torch


def _net(backbone):
    from cosa_amd.models import build_model
    from cosa_amd.train_step import default_args
    return build_model(default_args("VOC12", crop_size=64, backbone=backbone))


@pytest.mark.parametrize("backbone", ["vit_base_patch16_224", "dino_base_patch8_224"])
def test_fp32_mode_string_and_operand_map(backbone):
    """"fp32" is accepted for both built backbones; every projection of the map is "f32"; no x3 / c8 / c4 weight set has a member (the
    weights are the fp32 masters); the network's compute dtype is fp32, so no 16-bit shadow is made for it"""
    net = _net(backbone)
    net.check_nograd_precision("fp32")
    assert net.set_nograd_precision("fp32") is net
    enc = net.encoder
    assert enc.precision == "f32" and enc.compute_dtype == torch.float32 and net.compute_dtype == torch.float32
    fmap = enc._operand_map()
    depth = len(enc.blocks)
    assert fmap.patch == "f32" and fmap.attn == ("f32",) * depth and fmap.mlp == ("f32",) * depth
    assert fmap.dt16 is None and fmap.hdt is None and not fmap.plain_qkv and not fmap.c4_proj
    assert all(fmap.of(i, n) == "f32" for i in range(depth) for n in ("qkv", "proj", "fc1", "fc2"))
    assert fmap.uses("f32") and not any(fmap.uses(f) for f in ("plain", "x3", "c8", "c4"))
    for fmt in ("x3", "c8", "c4"):
        assert enc._operand_items(fmap, fmt) == []
    # leaving the mode leaves nothing behind
    net.set_nograd_precision("fp16x3")
    assert enc.precision == "bf16x3" and enc.compute_dtype == torch.float16 and enc._operand_map().patch == "x3"
    net.set_nograd_precision("bf16")
    assert enc.precision is None and enc.compute_dtype == torch.bfloat16 and enc._operand_map().patch == "plain"


@pytest.mark.parametrize("bad", ["fp32-3", "fp32-x2", "fp32-", "fp32-9m7", "fp32-c6", "fp32x3"])
def test_fp32_mode_takes_no_suffix(bad):
    """mixed maps are refused: an fp32 pass is fp32 from the patch projection to the heads"""
    net = _net("vit_base_patch16_224")
    net.set_nograd_precision("fp32")
    with pytest.raises(AssertionError):
        net.set_nograd_precision(bad)
    assert net.encoder.precision == "f32"          # (a refused string changes nothing)


def test_defaults_did_not_move_and_flags_accept_fp32():
    from cosa_amd import args as launcher_args, predict
    from cosa_amd.train_step import default_args, resolve_teacher_check_mode, resolve_teacher_precision
    assert [resolve_teacher_precision("auto", c) for c in (224, 448, 512, 640)] == ["fp16x3"] * 4
    assert resolve_teacher_precision("auto", 448, usepar=True) == "fp16x3" and resolve_teacher_precision("fp32", 448) == "fp32"
    assert resolve_teacher_check_mode("auto", "fp16x3") == "bf16x3"
    for other in ("bf16", "fp16", "bf16x3", "fp16c8-x2", "fp16c4", "fp32"):
        assert resolve_teacher_check_mode("auto", other) == "fp16x3"
    assert resolve_teacher_check_mode("fp32", "fp16x3") == "fp32" and resolve_teacher_check_mode("fp32", "fp32") == "fp32"
    a, changed = launcher_args.parse(["EXP", "--teacher_precision", "fp32", "--teacher_check_iters", "50", "--teacher_check_mode", "fp32"])
    assert a.teacher_precision == "fp32" and a.teacher_check_mode == "fp32" and changed["teacher_precision"] == "fp32"
    p, _ = predict.parse(["EXP", "--checkpoint", "x.pth", "--out", "o", "--teacher_precision", "fp32", "--teacher_check_mode", "fp32"])
    assert p.teacher_precision == "fp32" and p.teacher_check_mode == "fp32"
    d = default_args("VOC12", crop_size=64)
    assert d.teacher_precision == "auto" and d.teacher_check_mode == "auto"
    # what the flags name is a mode the network takes (the strings alone parse on any tree)
    _net("vit_base_patch16_224").set_nograd_precision(a.teacher_precision).set_nograd_precision(p.teacher_check_mode)


def test_host_trainer_accepts_fp32_modes():
    """a trainer on the host (no device teacher) takes --teacher_precision fp32 and an fp32 check mode through the same set-up checks"""
    from cosa_amd.train_step import CoSATrainer, default_args
    tr = CoSATrainer(default_args("VOC12", crop_size=64, teacher_precision="fp32", teacher_check_iters=2, teacher_check_mode="fp32"),
                     torch.device("cpu"), seed=1)
    assert tr.args.teacher_precision == "fp32" and tr.args.teacher_check_mode == "fp32"
    assert tr._teacher_shadows is None and tr.model_CK is None and tr.teacher_check_state is not None


def test_binding_declares_the_f32_entry_points():
    from cosa_amd import _C
    for s in ("cosa_gemm_f32", "cosa_attn_fwd_f32", "cosa_conv3x3_dilated_f32", "cosa_layernorm_f32out", "cosa_im2col_flip_f32_tokens"):
        assert s in _C.declared_symbols()
