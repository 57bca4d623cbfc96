"""CameraHeadTrainer's conv-stack opt-in without a GPU: which state-dict tensors it trains, the reference's norm / non-norm weight-decay
split (train_NopeSAC.py:88-135), and the argument checks of the conv-stack backward entry points (csrc/conv_bwd.hip)."""
import ctypes

import pytest
import torch

from nopesac_amd import _lib
from nopesac_amd.synth import synth_state_dict
from nopesac_amd.training import CameraHeadTrainer, is_norm_parameter

PFX = "camera_head_list.0."


def _expected_conv_stack_keys():
    keys = []
    for nm in ("adapter_1", "adapter_2", "layer_1", "layer_2", "layer_3"):
        keys += [f"pixel_decoder.{nm}.weight", f"pixel_decoder.{nm}.norm.weight", f"pixel_decoder.{nm}.norm.bias"]
    keys += ["pixel_decoder.mask_features.weight", "pixel_decoder.mask_features.bias"]
    for i in (0, 1, 3, 4, 6, 7):
        keys += [f"convs_backbone.{i}.0.weight", f"convs_backbone.{i}.1.weight", f"convs_backbone.{i}.1.bias"]
    for br in ("convs_trans", "convs_rots"):
        for i in range(6):
            keys += [f"{br}.{i}.0.weight", f"{br}.{i}.1.weight", f"{br}.{i}.1.bias"]
    return [PFX + k for k in keys]


def test_conv_stack_parameter_names():
    sd = synth_state_dict(50)
    base = CameraHeadTrainer.parameter_names(sd.keys())
    assert len(base) == 108
    full = CameraHeadTrainer.parameter_names(sd.keys(), conv_stacks=True)
    extra = _expected_conv_stack_keys()
    assert len(extra) == 71
    assert sorted(full) == sorted(base + extra) and len(full) == 179
    assert sum(k.endswith(".weight") and sd[k].dim() == 4 for k in extra) == 24
    assert not any(k.split(".")[-1] in ("running_mean", "running_var", "num_batches_tracked") for k in full)


def test_norm_weight_decay_split_follows_the_module_type_rule():
    """The reference gives WEIGHT_DECAY_NORM to parameters of GroupNorm / BatchNorm modules: pixel_decoder.*.norm.* (GroupNorm) and
    convs_*.i.1.* (BatchNorm2d) - and to nothing else of the camera head (conv weights, mask_features.bias, Linear layers)."""
    sd = synth_state_dict(50)
    full = CameraHeadTrainer.parameter_names(sd.keys(), conv_stacks=True)
    norm = {k for k in full if is_norm_parameter(k)}
    want = {k for k in full if (".norm." in k and k.startswith(PFX + "pixel_decoder.")) or
            (k[len(PFX):].split(".")[0] in ("convs_backbone", "convs_trans", "convs_rots") and k.split(".")[-2] == "1")}
    assert norm == want and len(norm) == 46
    assert not any(is_norm_parameter(k) for k in CameraHeadTrainer.parameter_names(sd.keys()))


def _lib_or_skip():
    try:
        return _lib.load()
    except RuntimeError as e:            # pragma: no cover - the library is built by build()
        pytest.skip(str(e))


def test_conv_backward_entry_points_reject_bad_arguments():
    """Every new entry point checks its arguments before any HIP call (NPS_E_ARG, no device needed)."""
    L = _lib_or_skip()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    E = -1
    # dgrad: null pointer, 5x5 kernel, stride 3, workspace too small for stride 1
    assert L.nopesac_conv2d_dgrad_f32(None, p, p, p, 256, 1, 4, 4, 4, 4, 3, 3, 1, 1, 4, 4, None) == E
    assert L.nopesac_conv2d_dgrad_f32(p, p, p, p, 1 << 20, 1, 8, 8, 4, 4, 5, 5, 1, 2, 4, 4, None) == E
    assert L.nopesac_conv2d_dgrad_f32(p, p, p, p, 1 << 20, 1, 8, 8, 4, 4, 3, 3, 3, 1, 4, 4, None) == E
    assert L.nopesac_conv2d_dgrad_f32(p, p, p, p, 16, 1, 8, 8, 4, 4, 3, 3, 1, 1, 4, 4, None) == E
    # wgrad: Cin % 4 != 0, splits 0, workspace too small
    assert L.nopesac_conv2d_wgrad_f32(p, p, p, p, 1 << 20, 1, 8, 8, 3, 4, 3, 3, 1, 1, 3, 4, 1, None) == E
    assert L.nopesac_conv2d_wgrad_f32(p, p, p, p, 1 << 20, 1, 8, 8, 4, 4, 3, 3, 1, 1, 4, 4, 0, None) == E
    assert L.nopesac_conv2d_wgrad_f32(p, p, p, p, 16, 1, 8, 8, 4, 4, 3, 3, 1, 1, 4, 4, 2, None) == E
    assert L.nopesac_conv2d_wgrad_workspace_bytes(128, 300, 3, 3, 4) == 4 * 128 * 300 * 9 * 4
    # BatchNorm + activation: sigmoid is not a supported activation, empty rows, small workspace
    assert L.nopesac_bn_act_forward_f32(p, p, p, p, p, 1e-3, 3, 4, 4, p, None) == E
    assert L.nopesac_bn_act_backward_f32(p, p, p, p, p, p, 1e-3, 2, 0, 4, p, p, p, p, 64, None) == E
    assert L.nopesac_bn_act_backward_f32(p, p, p, p, p, p, 1e-3, 2, 1024, 4, p, p, p, p, 8, None) == E
    assert L.nopesac_bn_act_backward_workspace_floats(1024, 4) == 4 * 2 * 4
    # GroupNorm: channels not divisible by the groups, small workspace
    assert L.nopesac_groupnorm_backward_f32(p, p, p, p, 1, 4, 30, 32, 1e-5, 0, p, p, p, p, 64, None) == E
    assert L.nopesac_groupnorm_backward_f32(p, p, p, p, 2, 4, 64, 32, 1e-5, 0, p, p, p, p, 8, None) == E
    assert L.nopesac_maxpool2x2_backward_f32(p, p, p, 1, 1, 4, 4, None) == E
    assert L.nopesac_upsample2x_nearest_add_backward_f32(None, p, 1, 2, 2, 4, None) == E
    assert L.nopesac_corr_softmax_backward_f32(p, p, 1, 4, 8, 4, 8, p, p, None) == E
    assert L.nopesac_transpose_batched_f32(p, 0, 4, 4, p, None) == E


def test_ops_wrappers_validate_without_a_gpu():
    from nopesac_amd import ops
    x = torch.zeros(1, 4, 4, 8)
    with pytest.raises(ops.OpsArgumentError):
        ops.conv2d_dgrad(x, torch.zeros(8, 8, 3, 3), (4, 4), pad=1)        # CPU tensors: there is no CPU path
    with pytest.raises(ops.OpsArgumentError):
        ops.maxpool_backward(x, torch.zeros(1, 2, 2, 8))
