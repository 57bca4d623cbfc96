"""Training on MI355X, one trainer per module of the network (optimiser groups train_NopeSAC.py:88-169).  HeadTrainer is
the base of all of them and nothing else: it owns the f32 leaf parameters under their state-dict keys, the gradients (`grads`,
`input_grads` for the inputs a trainer watches), the sum-of-losses backward, the optimiser state and step (AdamW / SGD, global-norm
clipping, the reference's norm / embedding / plain groups stated once in parameter_group) and write_back into the inference head; a
subclass names its state-dict prefix (KEY_PREFIX) and its SOLVER.*_MULTIPLIER (LR_MULTIPLIER) and adds its forward.  ChainedTrainer adds
the protocol of a trainer whose output feeds the instance heads: forward, then backward_from(gradient at the output), or
losses(heads, ...) followed by backward.  The trainers: RefineTrainer (with CameraHeadTrainer on top of it), MatchingHeadTrainer,
PlaneInstanceHeadsTrainer, the chained PlaneDecoderTrainer, PlanePyramidTrainer and PlaneEncoderTrainer, and BackboneTrainer.

RefineTrainer is the camera head's refinement stage (reference: `__forward_PlaneCamRefHead`, camera_net/camera_head.py:737-923; losses
camera_modules.py:355-365) - round 5.  Forward = the kernels of the training-side twin (ops.geo_sequence, ops.ransac_score_maps, ops.ransac_soft_vote mode | 16,
ops.plane_cam_ref_losses) with the MLP stacks as one f32 GEMM launch per layer (every layer output is kept for the backward pass);
backward = the hand-written vector-Jacobian kernels of csrc/refine_bwd.hip (losses, scoring + aggregation + pose heads, hypothesis x
plane geometry) and, for every Linear layer, dgrad = dY W and wgrad = dY^T X on the library's f32 GEMM kernel + column sums for the
bias + the ReLU mask.  `torch.autograd.Function` only does the bookkeeping (which gradient goes where); concatenations and the
broadcast of the initial-pose features are torch views / a [B, nq, 256] sum.  Everything is f32 and deterministic.

The pixel pose net's conv stacks (pixel decoder, convs_backbone, the two strided branches, the correlation softmax between them) are
trainable on request: CameraHeadTrainer(conv_stacks=True) runs them from the trainer's own f32 parameters through the autograd Functions
below, whose backward passes are the kernels of csrc/conv_bwd.hip (conv dgrad / wgrad, BatchNorm + LeakyReLU, GroupNorm, max-pool,
upsample-add, correlation softmax).  By default BatchNorm runs with its stored statistics and a trainable affine (detectron2's
FrozenBatchNorm2d regime, as forward_train).  batch_stats=True trains the 18 conv + nn.BatchNorm2d + LeakyReLU blocks as the reference
does (camera_modules.py:36-48, never frozen): on BATCH statistics - per view in the siamese tower, which the reference calls once per
view - with the backward through them and the running buffers and counters updated on the device (csrc/camera_bn_train.hip).

The matching head (matching_net/matching_head.py:43-139: planeApp_proj, the 18 GNN layers, planeDesc_proj, the Sinkhorn with its
bin_score and the embedding loss) is trained by MatchingHeadTrainer: the forward is the unfused f32 route of modeling/matching_head.py
(ops.linear, ops.attention with lengths, ops.layernorm with addend, ops.matcher_sinkhorn) from the trainer's own parameters, launch for
launch - the same parameters give the inference head's log scores bit for bit; the backward is the kernels of csrc/matcher_bwd.hip
(ragged attention, LayerNorm, the unrolled Sinkhorn + loss, the descriptor dot) plus the Linear dgrad / wgrad above.

The plane head's set criterion (modeling/matcher.py HungarianMatcher + modeling/criterion.py SetCriterion, as forward_single calls them) is
PlaneCriterion: targets preparation, the matcher's cost matrices, the Hungarian match and the nine detection losses of every supervised
decoder layer run on the device (csrc/plane_criterion.hip) with no host round trip, and their gradients with respect to the head's
outputs (class logits, low-resolution mask logits, centres, parameters, the pixel centre map) come back through one autograd Function.
plane_corr_matrix turns the match of both views into the gt_corr MatchingHeadTrainer.matching_losses takes.

The plane head's instance heads (planeTR_head.py:146-192: plane_embedding, pixel_embedding, plane_prob, plane_param, plane_center,
pixel_plane_center - 24 tensors) are trained against that criterion by PlaneInstanceHeadsTrainer, under deep supervision: its inputs are
the two tensors where the head's trunk ends (PlaneTRHead.training_inputs: the supervised decoder outputs hs and the pixel decoder's map
p1), its forward makes the inference head's f32 launches for every supervised layer (the mask logits in folded form: the pixel-embedding
map is never materialised), and the backward of the mask product is the two MFMA launches of csrc/plane_head_bwd.hip.

The plane head's transformer decoder (planeTR_head.py:88, transformer/transformer.py:114-153, 293-322: six pre-norm layers with
dropout 0.1, the final norm, query_embed - 111 tensors) is trained by PlaneDecoderTrainer: it takes the instance heads' gradient at hs
(backward_from, or chained through one graph by losses / backward), runs the inference head's own launches at p = 0 and, at p > 0, the
kernels of csrc/decoder_train.hip - attention with dropout on the probabilities for any key count and its recomputing backward, and
element-wise dropout whose mask is a counter-based function of (seed, step, layer, site, element index) that is never stored.

The plane head's top-down pyramid (planeTR_head.py:209-252: eight conv1x1 + nn.BatchNorm2d + ReLU blocks, three of them behind a
bilinear 2x upsampling - 24 parameters, 16 running-statistics buffers, eight counters) is trained by PlanePyramidTrainer as the reference
trains it: BatchNorm on BATCH statistics with the running buffers updated on the device.  It takes the instance heads' gradient at p1
(backward_from, or chained by losses / backward), and its kernels are csrc/pyramid_train.hip - statistics, apply and backward of a
training-mode BatchNorm whose input is a matrix or the on-the-fly upsampling of a low-resolution map (the up convs stay at the low
resolution, as in the inference head), with the bilinear adjoint gathered inside the backward's second launch.  The encoder memory is a
shared input of this trainer and the decoder's: given the same leaf, autograd sums both paths.

The plane head's transformer encoder (planeTR_head.py:77-82, 125-132, transformer/transformer.py:183-199: input_proj, six post-norm
layers with dropout 0.1, the final norm - 76 tensors) is trained by PlaneEncoderTrainer, which takes the sum of the decoder's and the
pyramid's gradients at the memory (backward_from) or chains all four plane-head trainers through one graph (losses / backward: the 235
tensors of sem_seg_head).  Its Linears run on B x 300 rows, so their backward is _LinearInPlace: one call of ops.linear_backward
(csrc/linear_bwd.hip) that reads x, the gradient and the saved output where they lie - the ReLU and the counter-based dropout behind
the Linear are gates applied as the gradient's tiles are loaded - instead of _Linear's ReLU pass, three transposes, two GEMMs and a
column sum.  _Linear and the trainers that use it are unchanged.

The ResNet-50 backbone (configs/Base.yaml: FREEZE_AT 0, FrozenBN, SOLVER.BACKBONE_MULTIPLIER 0.1 - the 53 conv weights) is trained by
BackboneTrainer: its forward is the inference backbone's f32 launches (conv + FrozenBN + residual + ReLU in one epilogue), of which only
the post-activation outputs are kept; the backward is csrc/backbone_bwd.hip - the FrozenBN / ReLU gate from the saved output, the
input gradient of the six stride-2 convs as four parity-class GEMMs on the f32 MFMA, the stem's overlapping max-pool - plus the
stride-1 dgrad and the wgrad of csrc/conv_bwd.hip.  It takes the gradients the other trainers report at the backbone maps
(`input_grads`, through backward_from) or continues their graph (joined_backward), so one optimiser step can move every trainable
tensor of the model.

One optimiser step over SEVERAL trainers belongs to nopesac_amd/optim.py: ModelOptimizer clips the gradient norm over all of their
parameters (the reference's full-model clip - HeadTrainer.clip_grad_norm sees one trainer's), keeps one step counter, follows the
WarmupMultiStepLR schedule, averages gradients across ranks and saves / resumes its state, in a fixed number of launches.
HeadTrainer.step_from_cfg remains the single-trainer form, and the yardstick that ModelOptimizer is held to bit for bit.

The two-view half of the training forward (siamese_planeTR.py:237-299: the plane head's outputs of both views feed the matching head
and the camera head, nothing detached on the way) is TwoViewLosses: the matched queries of every image are gathered to a prefix on the
device (csrc/two_view_train.hip: match_compact, its scatter back, corr_compact) for MatchingHeadTrainer, and the camera head's `_Aux`
passes run with the PREDICTED planes on the tape (plane_grads: _GeoSequence around ops.geo_sequence, and the geo_local cotangent of
_ScoreMaps - the two backward kernels of the same file), so the refinement losses reach plane_param and, through hs, the decoder.
joint_backward is one backward over several trainers; ModelOptimizer steps them.

What this is NOT: the driver from images to an optimiser step - one forward of the meta-architecture in training mode that calls every
trainer - each trainer (and TwoViewLosses) is called by its user.  The image and the backbone maps are inputs of the stages, as they are
of the reference functions, and receive no gradient beyond `input_grads`; the assignment between the matcher and the camera head is
discrete and carries none.  Gated
against torch.autograd on the oracle (tests/test_training_gpu.py, tests/test_pose_net_training_gpu.py, tests/test_matcher_training_gpu.py)
and against float64 restatements pinned to the reference (tests/test_plane_criterion_gpu.py, tests/test_plane_heads_training_gpu.py, tests/test_plane_decoder_training_gpu.py, tests/test_plane_pyramid_training_gpu.py, tests/test_plane_encoder_training_gpu.py, tests/test_backbone_training_gpu.py)."""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from . import ops
from .ops import _require, col_sum, transpose_rows as transpose      # ([rows, cols] f32, rows may be strided: column sums / the transpose)

PREFIX = "camera_head_list.0."
CONV_STACKS = ("pixel_decoder", "convs_backbone", "convs_trans", "convs_rots")       # the pixel pose net's conv stacks (conv_stacks=True)
BACKBONE_CONVS = (0, 1, 3, 4, 6, 7)
BN_EPS, GN_EPS, GN_GROUPS = 1e-3, 1e-5, 32
BN_MOMENTUM = 0.01                     # nn.BatchNorm2d(eps=0.001, momentum=0.01) of the pixel pose net's conv blocks (camera_modules.py:45)
_BUFFER_LEAVES = ("running_mean", "running_var", "num_batches_tracked")


MATCHER_PREFIX = "matching_head."
GNN_LAYERS, GNN_HEADS, LN_EPS = 18, 8, 1e-5

PLANE_PREFIX = "sem_seg_head."
DECODER, TOP_DOWN = "context2plane_decoder", "top_down"              # the plane head's transformer decoder and top-down pyramid
ENCODER, INPUT_PROJ = "context_SA", "input_proj"                     # its transformer encoder and the 1x1 conv on res5 in front of it


def is_norm_parameter(key: str) -> bool:
    """GroupNorm / BatchNorm affine tensors of the camera head (the modules the reference's build_optimizer gives WEIGHT_DECAY_NORM,
    train_NopeSAC.py:94-128): pixel_decoder.*.norm.{weight,bias} and convs_*.i.1.{weight,bias}; and the LayerNorm affine tensors of the
    matching head's GNN (torch.nn.LayerNorm is one of the reference's norm_module_types, train_NopeSAC.py:106):
    matching_head.gnn.layers.N.norm{1,2}.{weight,bias}."""
    if key.startswith(MATCHER_PREFIX):
        parts = key[len(MATCHER_PREFIX):].split(".")
        return len(parts) == 5 and parts[:2] == ["gnn", "layers"] and parts[3] in ("norm1", "norm2") and parts[4] in ("weight", "bias")
    parts = key[len(PREFIX):].split(".") if key.startswith(PREFIX) else key.split(".")
    if parts[0] == "pixel_decoder":
        return len(parts) == 4 and parts[2] == "norm"
    if parts[0] in CONV_STACKS:
        return len(parts) == 4 and parts[2] == "1" and parts[3] in ("weight", "bias")
    return False


def parameter_group(key: str) -> str:
    """The optimiser group of a state-dict key, "norm", "embed" or "plain" (the reference's build_optimizer, train_NopeSAC.py:88-135:
    norm module types take WEIGHT_DECAY_NORM, nn.Embedding WEIGHT_DECAY_EMBED).  Under sem_seg_head.: query_embed is the embedding, the
    decoder's and the encoder's LayerNorms (norm, norm1-3 / context_SA's norm, norm1-2) and the BatchNorm of every pyramid block (conv_bn_relu: Sequential(0 = conv, 1 = BatchNorm2d,
    2 = ReLU)) are norms, the instance heads have neither; the camera head and the matcher: is_norm_parameter."""
    if key.startswith(PLANE_PREFIX):
        parts = key[len(PLANE_PREFIX):].split(".")
        if parts[0] == "query_embed":
            return "embed"
        norm = ((parts[0] == DECODER and parts[-2] in ("norm", "norm1", "norm2", "norm3")) or (parts[0] == TOP_DOWN and parts[-2] == "1")
                or (parts[0] == ENCODER and parts[-2] in ("norm", "norm1", "norm2")))
        return "norm" if norm else "plain"
    return "norm" if is_norm_parameter(key) else "plain"


MLPS = ("geo_encoder", "geo_proj_s1", "decoder_rot", "geo_proj_s2", "decoder_tran", "decoder_rot2", "decoder_tran2", "normal_score_proj",
        "param_score_proj")
LINEARS = ("rots", "trans", "rot_score_reg", "trans_score_reg")
_ACT_BACKWARD = {ops.ACT_NONE: None, ops.ACT_RELU: ops.relu_backward, ops.ACT_SIGMOID: ops.sigmoid_backward}      # of _Linear's epilogues


class _Linear(torch.autograd.Function):
    """y = act(x W^T + b [+ residual]) on the exact-f32 GEMM kernel, act (ops.ACT_NONE / ACT_RELU / ACT_SIGMOID) and the residual in the
    GEMM's epilogue as the inference heads launch them; backward: the activation's first (it reads y, which is saved only then), then
    dX = dY W, dW = dY^T X (the same kernel), db = column sums of the gradient dY in front of the activation, which is the residual's."""

    @staticmethod
    def forward(ctx, x, w, b, act: int, residual):
        _require(act in _ACT_BACKWARD, act)
        x = x.contiguous()
        y = ops.linear(x, w, b, act=act, residual=None if residual is None else residual.contiguous())
        ctx.act = act
        ctx.save_for_backward(x, w, *(() if _ACT_BACKWARD[act] is None else (y,)))
        return y

    @staticmethod
    def backward(ctx, g):
        x, w, *y = ctx.saved_tensors
        g = g.contiguous()
        if y:
            g = _ACT_BACKWARD[ctx.act](g, y[0])
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = ops.linear(g, transpose(w))                      # [rows, N] x [N, K]
        if ctx.needs_input_grad[1]:
            gw = ops.linear(transpose(g), transpose(x))           # [N, rows] x [rows, K]
        if ctx.needs_input_grad[2]:
            gb = col_sum(g)
        return gx, gw, gb, None, (g if ctx.needs_input_grad[4] else None)


def _linear(x, w, b=None, act: int = ops.ACT_NONE, residual=None):
    return _Linear.apply(x, w, b, act, residual)


def _in_place_operand(t: torch.Tensor) -> torch.Tensor:
    """t as ops.linear_backward reads it in place: rows of unit column stride, 16-byte aligned, a row stride that is a multiple of 4
    (a column slice of a wider buffer qualifies); anything else is made dense."""
    ok = t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1] and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0
    return t if ok else t.contiguous()


class _LinearInPlace(torch.autograd.Function):
    """_Linear with the backward as ONE call of ops.linear_backward (csrc/linear_bwd.hip): no ReLU pass, no transposes, no column-sum
    launch - x, the gradient and the saved output are read where they lie and the gates are applied as the tiles are loaded.  The
    forward is _Linear's ops.linear launch (act: ops.ACT_NONE or ACT_RELU; a residual goes into the GEMM's epilogue), so the forward
    bits are _Linear's.  p > 0: the dropout that sits directly behind the Linear is part of the Function -
    out = ops.dropout(act(x W^T + b), p, seed, stream) + residual - and its mask is the backward call's second gate, recomputed from
    the counter.  The residual's gradient is the incoming one."""

    @staticmethod
    def forward(ctx, x, w, b, act: int, residual, p: float, seed: int, stream: int):
        _require(act in (ops.ACT_NONE, ops.ACT_RELU), act)
        _require(residual is None or act == ops.ACT_NONE, "_LinearInPlace: a residual goes with ACT_NONE")
        x = x.contiguous()
        res = None if residual is None else residual.contiguous()
        if p == 0.0:
            h = out = ops.linear(x, w, b, act=act, residual=res)
        else:
            h = ops.linear(x, w, b, act=act)
            out = ops.dropout(h, p, seed, stream, residual=res)
        ctx.conf = (float(p), int(seed), int(stream))
        ctx.save_for_backward(x, w, *((h,) if act == ops.ACT_RELU else ()))
        return out

    @staticmethod
    def backward(ctx, g):
        x, w, *y = ctx.saved_tensors
        p, seed, stream = ctx.conf
        g = _in_place_operand(g)
        want = tuple(ctx.needs_input_grad[:3])
        gx = gw = gb = None
        if any(want):
            gx, gw, gb = ops.linear_backward(x.view(-1, x.shape[-1]), w, g.view(-1, g.shape[-1]) if g.dim() != 2 else g,
                                             y=y[0].view(-1, y[0].shape[-1]) if y else None, p=p, seed=seed, stream=stream, want=want)
            gx = None if gx is None else gx.view(x.shape)
        return gx, gw, gb, None, (g if ctx.needs_input_grad[4] else None), None, None, None


def _mlp_stack(P: Dict[str, torch.Tensor], q: str, x, last_act: int = ops.ACT_NONE):
    """The MLP under the key prefix q (`q.layers.i.{weight,bias}`): ReLU between the layers, last_act behind the last one."""
    i = 0
    while f"{q}.layers.{i + 1}.weight" in P:
        x = _linear(x, P[f"{q}.layers.{i}.weight"], P[f"{q}.layers.{i}.bias"], ops.ACT_RELU)
        i += 1
    return _linear(x, P[f"{q}.layers.{i}.weight"], P[f"{q}.layers.{i}.bias"], last_act)


class _GeoSequence(torch.autograd.Function):
    """ops.geo_sequence with the PLANES on the tape (plane_grads): (geo_local, geo_enc, m), the backward is one launch of
    ops.geo_sequence_backward.  The pose is a constant, as in the reference (the detached initial pose, camera_head.py:353-368)."""

    @staticmethod
    def forward(ctx, A0, planes1, planes2, n1, n2, init_trans, init_rot, warp_in_ref: bool):
        planes1, planes2 = planes1.contiguous(), planes2.contiguous()
        geo_local, _gg, _sig, geo_enc, m = ops.geo_sequence(A0, planes1, planes2, n1, n2, init_trans, init_rot, warp_in_ref)
        ctx.warp_in_ref = bool(warp_in_ref)
        ctx.save_for_backward(A0, planes1, planes2, n1, n2, init_trans, init_rot)
        ctx.mark_non_differentiable(m)
        return geo_local, geo_enc, m

    @staticmethod
    def backward(ctx, g_local, g_enc, _m):
        A0, planes1, planes2, n1, n2, init_trans, init_rot = ctx.saved_tensors
        B, nq, _ = A0.shape
        z = lambda t, d: torch.zeros(B, nq, d, device=A0.device, dtype=torch.float32) if t is None else t.contiguous()
        g1, g2 = ops.geo_sequence_backward(A0, planes1, planes2, n1, n2, init_trans, init_rot, z(g_local, 6), z(g_enc, 8), ctx.warp_in_ref)
        return None, g1, g2, None, None, None, None, None


class _ScoreMaps(torch.autograd.Function):
    @staticmethod
    def forward(ctx, geo_local, rot_raw, trans_raw, init_rot, init_trans, m):
        out = ops.ransac_score_maps(geo_local, rot_raw.contiguous(), trans_raw.contiguous(), init_rot, init_trans, m, diagnostics=True)
        ctx.save_for_backward(geo_local, rot_raw, trans_raw, init_rot, init_trans, m)
        # (rots_all / trans_all only pick the hypothesis of the index losses; the row sums feed the inference-only 'min-cost' mode)
        ctx.mark_non_differentiable(out["rots_all"], out["trans_all"], out["dn_sum"], out["dl2_sum"])
        return out["normal_score"], out["param_score"], out["l2_dist"], out["rots_all"], out["trans_all"], out["dn_sum"], out["dl2_sum"]

    @staticmethod
    def backward(ctx, g_ns, g_ps, g_l2, _a, _b, _c, _d):
        geo_local, rot_raw, trans_raw, init_rot, init_trans, m = ctx.saved_tensors
        B, nq, _ = geo_local.shape
        z = lambda t, ref: torch.zeros_like(ref) if t is None else t.contiguous()
        ref = torch.empty(B, nq + 1, nq, device=geo_local.device, dtype=torch.float32)
        g_ns, g_ps, g_l2 = (z(t, ref) for t in (g_ns, g_ps, g_l2))
        g_rot, g_tr, g_ir, g_it = ops.ransac_score_maps_backward(geo_local, rot_raw.contiguous(), trans_raw.contiguous(), init_rot, init_trans, m,
                                                                 g_ns, g_ps, g_l2)
        g_geo = None
        if ctx.needs_input_grad[0]:                               # (plane_grads: geo_local comes from _GeoSequence)
            g_geo = ops.ransac_score_maps_backward_geo(geo_local, rot_raw.contiguous(), trans_raw.contiguous(), init_rot, init_trans, m,
                                                       g_ns, g_ps, g_l2)
        return g_geo, g_rot, g_tr, g_ir, g_it, None


class _Vote(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sf_rot, sf_trans, reg_rot_w, reg_rot_b, reg_trans_w, reg_trans_b, init_rot_feat, init_trans_feat, fused_rot, fused_trans,
                rots_w, rots_b, trans_w, trans_b, rots_all, trans_all, dn_sum, dl2_sum, init_rot, init_trans, m):
        args = [t.contiguous() for t in (sf_rot, sf_trans, reg_rot_w, reg_rot_b, reg_trans_w, reg_trans_b, init_rot_feat, init_trans_feat, fused_rot,
                                         fused_trans, rots_w, rots_b, trans_w, trans_b)]
        maps = {"rots_all": rots_all, "trans_all": trans_all, "dn_sum": dn_sum, "dl2_sum": dl2_sum}
        out = ops.ransac_soft_vote(*args, maps, init_rot, init_trans, m, 16)
        ctx.save_for_backward(*args, m)
        return out["pred_rot"], out["pred_trans"], out["avg_rot"], out["avg_trans"], out["score_rot"], out["score_trans"]

    @staticmethod
    def backward(ctx, g_pr, g_pt, g_ar, g_at, g_sr, g_st):
        (sf_rot, sf_trans, reg_rot_w, reg_rot_b, reg_trans_w, reg_trans_b, init_rot_feat, init_trans_feat, fused_rot, fused_trans, rots_w, rots_b,
         trans_w, trans_b, m) = ctx.saved_tensors
        B, NH, _ = sf_rot.shape
        nq = NH - 1
        dev = sf_rot.device
        f32 = dict(device=dev, dtype=torch.float32)
        zl = lambda t, shape: torch.zeros(shape, **f32) if t is None else t.contiguous()
        g_pr, g_ar = zl(g_pr, (B, 4)), zl(g_ar, (B, 4))
        g_pt, g_at = zl(g_pt, (B, 3)), zl(g_at, (B, 3))
        g_sr, g_st = zl(g_sr, (B, NH)), zl(g_st, (B, NH))
        o = ops.ransac_soft_vote_backward(sf_rot, sf_trans, reg_rot_w, reg_rot_b, reg_trans_w, reg_trans_b, init_rot_feat, init_trans_feat, fused_rot,
                                          fused_trans, rots_w, rots_b, trans_w, trans_b, m, g_pr, g_pt, g_ar, g_at, g_sr, g_st)
        red = lambda t, like: col_sum(t).view_as(like)              # per-pair partials -> the parameter's gradient (fixed order)
        return (o["g_sf_rot"], o["g_sf_trans"], red(o["pb_reg_rot_w"], reg_rot_w), red(o["pb_reg_rot_b"], reg_rot_b),
                red(o["pb_reg_trans_w"], reg_trans_w), red(o["pb_reg_trans_b"], reg_trans_b), o["g_init_rot_feat"], o["g_init_trans_feat"],
                o["g_fused_rot"], o["g_fused_trans"], red(o["pb_rots_w"], rots_w), red(o["pb_rots_b"], rots_b), red(o["pb_trans_w"], trans_w),
                red(o["pb_trans_b"], trans_b), None, None, None, None, None, None, None)


class _Losses(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred_rot, pred_trans, avg_rot, avg_trans, score_rot, score_trans, l2_dist, rots_all, trans_all, m, gt_pose, weight: float):
        vote = {"pred_rot": pred_rot.contiguous(), "pred_trans": pred_trans.contiguous(), "avg_rot": avg_rot.contiguous(), "avg_trans": avg_trans.contiguous(),
                "score_rot": score_rot.contiguous(), "score_trans": score_trans.contiguous()}
        maps = {"rots_all": rots_all, "trans_all": trans_all, "l2_dist": l2_dist.contiguous()}
        ctx.weight = float(weight)
        ctx.save_for_backward(vote["pred_rot"], vote["pred_trans"], vote["avg_rot"], vote["avg_trans"], vote["score_rot"], vote["score_trans"], rots_all,
                              trans_all, m, gt_pose)
        return ops.plane_cam_ref_losses(vote, maps, m, gt_pose, weight)

    @staticmethod
    def backward(ctx, g):
        pr, pt, ar, at, sr, st, rots_all, trans_all, m, gt = ctx.saved_tensors
        vote = {"pred_rot": pr, "pred_trans": pt, "avg_rot": ar, "avg_trans": at, "score_rot": sr, "score_trans": st}
        grads = ops.plane_cam_ref_losses_backward(vote, {"rots_all": rots_all, "trans_all": trans_all}, m, gt, g.contiguous(), ctx.weight)
        return (*grads, None, None, None, None, None)


class _Normalize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, canonical: bool):
        x = x.contiguous()
        ctx.canonical = bool(canonical)
        ctx.save_for_backward(x)
        return ops.normalize_rows(x, canonical_sign=ctx.canonical)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return ops.normalize_rows_backward(x, g.contiguous(), ctx.canonical), None


class _PoseLoss(torch.autograd.Function):
    """CameraPoseLoss / the AIM's reconstruction losses (ops.camera_pose_loss) -> f32[2] = (l_x, l_q) * weight."""

    @staticmethod
    def forward(ctx, est_t, est_q, gt_t, gt_q, weight: float, trans_eps: float):
        est_t, est_q, gt_t, gt_q = (t.contiguous() for t in (est_t, est_q, gt_t, gt_q))
        ctx.weight, ctx.eps = float(weight), float(trans_eps)
        ctx.save_for_backward(est_t, est_q, gt_t, gt_q)
        return ops.camera_pose_loss(est_t, est_q, gt_t, gt_q, weight, trans_eps)

    @staticmethod
    def backward(ctx, g):
        est_t, est_q, gt_t, gt_q = ctx.saved_tensors
        return (*ops.camera_pose_loss_backward(est_t, est_q, gt_t, gt_q, g.contiguous(), ctx.weight, ctx.eps), None, None)


def _ohwi(w: torch.Tensor, cin: int) -> torch.Tensor:
    """State-dict conv weight [Cout, Cin, KH, KW] -> the forward conv's operand [Cout, KH, KW, cin] (zero channels beyond Cin)."""
    w = w.detach().permute(0, 2, 3, 1)
    if cin > w.shape[-1]:
        w = torch.nn.functional.pad(w, (0, cin - w.shape[-1]))
    return w.contiguous()


def _conv_input_grads(ctx, x, w, dc, stride: int, pad: int):
    """dX (zero in x's padding channels) and dW of a conv whose output gradient is dc."""
    dx = dw = None
    B, H, W, Cx = x.shape
    Cin = w.shape[1]
    if ctx.needs_input_grad[0]:
        dx = torch.zeros_like(x) if Cx > Cin else torch.empty_like(x)
        ops.conv2d_dgrad(dc, w, (H, W), stride=stride, pad=pad, out=dx[..., :Cin] if Cx > Cin else dx)
    if ctx.needs_input_grad[1]:
        dw = ops.conv2d_wgrad(x, dc, w.shape[2], stride=stride, pad=pad, cin=Cin)
    return dx, dw


class _ConvBNAct(torch.autograd.Function):
    """conv (no bias) + inference-mode BatchNorm (trainable affine, stored statistics) + act; the raw conv output is saved."""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, mean, var, stride: int, pad: int, act: int):
        x = x.contiguous()
        c = ops.conv2d(x, _ohwi(w, x.shape[3]), stride=stride, pad=pad)
        ctx.conf = (stride, pad, act)
        ctx.save_for_backward(x, w, c, gamma, beta, mean, var)
        return ops.bn_act_forward(c, gamma, beta, mean, var, BN_EPS, act)

    @staticmethod
    def backward(ctx, g):
        x, w, c, gamma, beta, mean, var = ctx.saved_tensors
        stride, pad, act = ctx.conf
        dc, dgamma, dbeta = ops.bn_act_backward(g.contiguous(), c, gamma, beta, mean, var, BN_EPS, act)
        dx, dw = _conv_input_grads(ctx, x, w, dc, stride, pad)
        return dx, dw, dgamma, dbeta, None, None, None, None, None


class _ConvBNActBatch(torch.autograd.Function):
    """conv (no bias) + training-mode BatchNorm on GROUPED batch statistics + LeakyReLU: the batch's rows are cut into `groups` runs of
    consecutive images, each normalised by its own mean and variance (the siamese tower: one run per view), and the running buffers
    take the runs' statistics in that order, in place (ops.bn_train_grouped_*).  The raw conv output is saved."""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, run_mean, run_var, stride: int, pad: int, groups: int):
        x = x.contiguous()
        c = ops.conv2d(x, _ohwi(w, x.shape[3]), stride=stride, pad=pad)
        mean, _var, rstd = ops.bn_train_grouped_stats(c, groups, eps=BN_EPS, momentum=BN_MOMENTUM, running_mean=run_mean, running_var=run_var)
        ctx.conf = (stride, pad, groups)
        ctx.save_for_backward(x, w, c, gamma, beta, mean, rstd)
        return ops.bn_train_grouped_apply(c, gamma, beta, mean, rstd, ops.ACT_LEAKY, groups)

    @staticmethod
    def backward(ctx, g):
        x, w, c, gamma, beta, mean, rstd = ctx.saved_tensors
        stride, pad, groups = ctx.conf
        dc, dgamma, dbeta = ops.bn_train_grouped_backward(g.contiguous(), c, gamma, beta, mean, rstd, ops.ACT_LEAKY, groups)
        dx, dw = _conv_input_grads(ctx, x, w, dc, stride, pad)
        return dx, dw, dgamma, dbeta, None, None, None, None, None


class _ConvGN(torch.autograd.Function):
    """d2 Conv2d (no bias) + GroupNorm(32) [+ ReLU] of the pixel decoder (camera_modules.py:271-303)."""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, pad: int, relu: bool):
        x = x.contiguous()
        c = ops.conv2d(x, _ohwi(w, x.shape[3]), pad=pad)
        ctx.conf = (pad, ops.ACT_RELU if relu else ops.ACT_NONE)
        ctx.save_for_backward(x, w, c, gamma, beta)
        return ops.groupnorm(c, gamma, beta, GN_GROUPS, GN_EPS, ctx.conf[1])

    @staticmethod
    def backward(ctx, g):
        x, w, c, gamma, beta = ctx.saved_tensors
        pad, act = ctx.conf
        dc, dgamma, dbeta = ops.groupnorm_backward(c, g.contiguous(), gamma, beta, GN_GROUPS, GN_EPS, act)
        dx, dw = _conv_input_grads(ctx, x, w, dc, 1, pad)
        return dx, dw, dgamma, dbeta, None, None


class _ConvBias(torch.autograd.Function):
    """conv + bias (pixel_decoder.mask_features); bias gradient = column sums of dY."""

    @staticmethod
    def forward(ctx, x, w, b, pad: int):
        x = x.contiguous()
        ctx.pad = pad
        ctx.save_for_backward(x, w)
        return ops.conv2d(x, _ohwi(w, x.shape[3]), bias=b.detach().contiguous(), pad=pad)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g = g.contiguous()
        dx, dw = _conv_input_grads(ctx, x, w, g, 1, ctx.pad)
        db = col_sum(g.view(-1, g.shape[3])) if ctx.needs_input_grad[2] else None
        return dx, dw, db, None


class _MaxPool2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        ctx.save_for_backward(x)
        return ops.maxpool(x, 2, 2, 0)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return ops.maxpool_backward(x, g.contiguous())


class _UpsampleAdd(torch.autograd.Function):
    """lateral + nearest 2x upsampling of x (the pixel decoder's top-down path)."""

    @staticmethod
    def forward(ctx, x, lateral):
        return ops.upsample2x_nearest_add(x.contiguous(), lateral.contiguous())

    @staticmethod
    def backward(ctx, g):
        dx, dlat = ops.upsample2x_nearest_add_backward(g.contiguous())
        return dx, dlat


class _CorrSoftmax(torch.autograd.Function):
    """The correlation volume + softmax (camera_head.py:1117-1133) -> A [B, h, w, pad_to] (zero channels beyond h w)."""

    @staticmethod
    def forward(ctx, x1, x2, pad_to: int):
        x1, x2 = x1.contiguous(), x2.contiguous()
        a = ops.corr_softmax(x1, x2, pad_to)
        ctx.save_for_backward(a, x1, x2)
        return a

    @staticmethod
    def backward(ctx, g):
        a, x1, x2 = ctx.saved_tensors
        dx1, dx2 = ops.corr_softmax_backward(a, g.contiguous(), x1, x2)
        return dx1, dx2, None


class _Attention(torch.autograd.Function):
    """ops.attention (f32, head dim 32, ragged by qlen / klen) on row-major q / k / v that may be column slices of a wider matrix;
    backward: ops.attention_backward (softmax recomputed)."""

    @staticmethod
    def forward(ctx, q, k, v, B: int, Lq: int, Lk: int, heads: int, scale: float, qlen, klen):
        o = ops.attention(q, k, v, B, Lq, Lk, heads, scale, qlen, klen)
        ctx.conf = (B, Lq, Lk, heads, float(scale))
        ctx.save_for_backward(q, k, v, qlen, klen)
        return o

    @staticmethod
    def backward(ctx, g):
        q, k, v, qlen, klen = ctx.saved_tensors
        B, Lq, Lk, heads, scale = ctx.conf
        dq, dk, dv = ops.attention_backward(q, k, v, g.contiguous(), B, Lq, Lk, heads, scale, qlen, klen)
        return dq, dk, dv, None, None, None, None, None, None, None


class _AttentionFused(torch.autograd.Function):
    """The same attention on the projections as the inference head lays them out (MatchingHead._gnn_layer): a self layer passes
    q = None and packed = q|k|v [rows, 768], a cross layer q [rows, 256] and packed = k|v [rows, 512].  The kernels take the column
    slices as they are, and the backward writes dq / dk / dv straight into one gradient of the packed matrix."""

    @staticmethod
    def forward(ctx, q, packed, B: int, Lq: int, Lk: int, heads: int, scale: float, qlen, klen):
        W = heads * 32
        packed = packed.contiguous()
        if q is None:
            qv, kv, vv = packed[:, :W], packed[:, W:2 * W], packed[:, 2 * W:]
        else:
            q = q.contiguous()
            qv, kv, vv = q, packed[:, :W], packed[:, W:]
        o = ops.attention(qv, kv, vv, B, Lq, Lk, heads, scale, qlen, klen)
        ctx.conf = (B, Lq, Lk, heads, float(scale), q is None)
        ctx.save_for_backward(q, packed, qlen, klen)
        return o

    @staticmethod
    def backward(ctx, g):
        q, packed, qlen, klen = ctx.saved_tensors
        B, Lq, Lk, heads, scale, self_layer = ctx.conf
        W = heads * 32
        g = g.contiguous()
        dpacked = torch.empty_like(packed)
        if self_layer:
            dq = None
            qv, kv, vv = packed[:, :W], packed[:, W:2 * W], packed[:, 2 * W:]
            gq, gk, gv = dpacked[:, :W], dpacked[:, W:2 * W], dpacked[:, 2 * W:]
        else:
            dq = torch.empty_like(q)
            qv, kv, vv = q, packed[:, :W], packed[:, W:]
            gq, gk, gv = dq, dpacked[:, :W], dpacked[:, W:]
        ops.attention_backward(qv, kv, vv, g, B, Lq, Lk, heads, scale, qlen, klen, out=(gq, gk, gv))
        return dq, dpacked, None, None, None, None, None, None, None


class _LinearSplit(torch.autograd.Function):
    """y = relu([a | b] W^T) computed as the inference head computes mlp.0: a W[:, :Da]^T first, then b W[:, Da:]^T with the first
    product as the residual in front of the ReLU (two GEMMs, no concatenated copy).  Backward: that of _Linear on [a | b]
    (ops.concat_cols) - dgrad split into two column slices, wgrad in one GEMM."""

    @staticmethod
    def forward(ctx, a, b, w):
        a, b = a.contiguous(), b.contiguous()
        Da = a.shape[1]
        h = ops.linear(a, w[:, :Da].contiguous())
        y = ops.linear(b, w[:, Da:].contiguous(), residual=h, act=ops.ACT_RELU)
        ctx.Da = Da
        ctx.save_for_backward(a, b, w, y)
        return y

    @staticmethod
    def backward(ctx, g):
        a, b, w, y = ctx.saved_tensors
        gm = ops.relu_backward(g.contiguous(), y)
        ga = gb = gw = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            gx = ops.linear(gm, transpose(w))
            ga, gb = gx[:, :ctx.Da], gx[:, ctx.Da:]
        if ctx.needs_input_grad[2]:
            gw = ops.linear(transpose(gm), transpose(ops.concat_cols(a, b)))
        return ga, gb, gw


class _LayerNorm(torch.autograd.Function):
    """LayerNorm(x) gamma + beta over D = 256 [+ addend] (ops.layernorm); the addend's gradient is the incoming gradient."""

    @staticmethod
    def forward(ctx, x, gamma, beta, addend):
        x = x.contiguous()
        ctx.save_for_backward(x, gamma)
        if addend is None:
            return ops.layernorm(x, gamma, beta, eps=LN_EPS)
        return ops.layernorm(x, gamma, beta, addend=addend.contiguous(), eps=LN_EPS)[1]

    @staticmethod
    def backward(ctx, g):
        x, gamma = ctx.saved_tensors
        g = g.contiguous()
        dx, dgamma, dbeta = ops.layernorm_backward(x, gamma, g, LN_EPS)
        return dx, dgamma, dbeta, (g if ctx.needs_input_grad[3] else None)


class _DescDot(torch.autograd.Function):
    """dots[b] = D0[b] D1[b]^T / sqrt(256) on the batched-weights f32 GEMM (as MatchingHead.forward); backward:
    ops.desc_dot_backward over the live n1 x n2 block - padded descriptor rows get exactly zero."""

    @staticmethod
    def forward(ctx, d0, d1, n1, n2):
        d0, d1 = d0.contiguous(), d1.contiguous()
        B, nq, D = d0.shape
        scale = torch.full((nq,), 1.0 / D ** 0.5, device=d0.device, dtype=torch.float32)
        ctx.save_for_backward(d0, d1, n1, n2)
        return ops.conv2d(d0.view(B, 1, nq, D), d1.view(B, nq, 1, 1, D), scale, batched_weights=True).view(B, nq, nq)

    @staticmethod
    def backward(ctx, g):
        d0, d1, n1, n2 = ctx.saved_tensors
        dd0, dd1 = ops.desc_dot_backward(g.contiguous(), d0, d1, n1, n2)
        return dd0, dd1, None, None


class _SinkhornEmbLoss(torch.autograd.Function):
    """ops.matcher_sinkhorn + embedding_loss_forward (matching_head.py:135-139) -> (loss, log_scores_padded).  The forward IS the
    inference launch (its assignment output is dropped), so log_scores_padded are the inference head's scores bit for bit;
    loss = 2 * mean(-min(log_scores, 0)) over the entries gt_corr selects in the whole batch (nopesac_matcher_emb_loss).  The geometric
    terms are constants (detached in the reference, :98-99).  Backward: nopesac_matcher_sinkhorn_train replays the iterations and keeps
    every iteration's potentials (a workspace that lives only inside the backward pass), then the gradient of the unrolled iterations.
    DEVIATION: a batch that selects no entry gives loss 0 and zero gradients (the reference's mean of nothing is NaN)."""

    @staticmethod
    def forward(ctx, dots, bin_score, planes1, planes2, cam7, n1, n2, gt_corr, offset_mult: float, normal_mult: float, iters: int):
        dots, bin_score = dots.contiguous(), bin_score.contiguous()
        log_scores, _assignment = ops.matcher_sinkhorn(dots, planes1, planes2, cam7, n1, n2, bin_score, float(offset_mult), float(normal_mult),
                                                       int(iters), 0.0)
        _stats, loss = ops.matcher_emb_loss(log_scores, gt_corr, n1, n2)
        ctx.conf = (float(offset_mult), float(normal_mult), int(iters))
        ctx.save_for_backward(dots, bin_score, planes1, planes2, cam7, n1, n2, gt_corr)
        ctx.loss = loss
        ctx.mark_non_differentiable(log_scores)
        return loss[:1].view(()), log_scores

    @staticmethod
    def backward(ctx, g, _g_scores):
        dots, bin_score, planes1, planes2, cam7, n1, n2, gt_corr = ctx.saved_tensors
        offset_mult, normal_mult, iters = ctx.conf
        inputs = (dots, planes1, planes2, cam7, n1, n2, bin_score, offset_mult, normal_mult, iters, gt_corr)
        _scores, uv, _stats, _loss = ops.matcher_sinkhorn_train(*inputs)
        d_dots, d_bin = ops.matcher_sinkhorn_train_backward(*inputs, uv, ctx.loss, g.contiguous().view(1))
        return d_dots, col_sum(d_bin.view(-1, 1)).view_as(bin_score), None, None, None, None, None, None, None, None, None


class HeadTrainer:
    """What every trainer here is: a module's parameters as f32 leaf tensors under their state-dict keys (`params`), their gradients
    after a backward (`grads`, and `input_grads` for the inputs the forward watched), the optimiser (`state`, `steps`) and write_back.
    A subclass sets KEY_PREFIX (the state-dict prefix of its module, which the inference head's own keys lack), LR_MULTIPLIER (the name
    of the SOLVER.*_MULTIPLIER its learning rate carries, train_NopeSAC.py:122-129, or None) and parameter_names, and adds its forward."""

    KEY_PREFIX = ""
    LR_MULTIPLIER: Optional[str] = None

    def __init__(self, params: Dict[str, torch.Tensor]):
        self.params = {k: v.detach().clone().float().contiguous().requires_grad_(True) for k, v in params.items()}
        self.state: Dict[str, dict] = {}
        self.steps = 0
        self.grads: Dict[str, torch.Tensor] = {}
        self.input_grads: Dict[str, torch.Tensor] = {}
        self._inputs: Dict[str, torch.Tensor] = {}

    @classmethod
    def _read(cls, source, names, device=None) -> Dict[str, torch.Tensor]:
        """{key: tensor} of the state-dict keys `names`, from an inference head (its raw tensors) or from a state dict (moved to device)."""
        if hasattr(source, "raw"):
            return {k: source.raw(k[len(cls.KEY_PREFIX):]) for k in names}
        return {k: source[k].to(device) for k in names}

    @classmethod
    def _head_keys(cls, head) -> List[str]:
        return [cls.KEY_PREFIX + k for k in head._spec_keys]

    def write_back(self, head):
        """Copy the trained parameters (and what else `_written_back` names) into the inference head (its packed / folded / bf16 copies
        are rebuilt on the next forward)."""
        self._copy_into(head, self._written_back())

    def _written_back(self) -> Dict[str, torch.Tensor]:
        """The tensors write_back copies: the parameters; a trainer that updates buffers adds them."""
        return self.params

    def _copy_into(self, head, tensors: Dict[str, torch.Tensor]):
        with torch.no_grad():
            for k, t in tensors.items():
                head.raw(k[len(self.KEY_PREFIX):]).copy_(t)
        head.invalidate()

    # ---- backward
    def _watch(self, inputs: Dict[str, torch.Tensor]):
        """The inputs whose gradients `input_grads` reports after the backward.  A caller may chain its own graph in front: non-leaf
        inputs keep their gradient only on request, and `input_grads` promises it."""
        self._inputs = inputs
        for t in inputs.values():
            if t.requires_grad and not t.is_leaf:
                t.retain_grad()

    def _clear_grads(self):
        for p in self.params.values():
            p.grad = None
        for t in self._inputs.values():
            if t.requires_grad and t.is_leaf:
                t.grad = None

    def _collect(self) -> Dict[str, torch.Tensor]:
        """-> `grads` = {state-dict key: gradient} (zeros where none arrived); `input_grads` = that of every watched input that requires
        grad and has one."""
        self.input_grads = {k: t.grad for k, t in self._inputs.items() if t.requires_grad and t.grad is not None}
        self.grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in self.params.items()}
        return self.grads

    def backward(self, losses: Dict[str, torch.Tensor], loss_weights: Optional[Dict[str, float]] = None) -> Dict[str, torch.Tensor]:
        """d (sum of the losses, optionally weighted) / d parameters -> {state-dict key: gradient}."""
        self._clear_grads()
        total = None
        for k, v in losses.items():
            term = v * float(loss_weights.get(k, 1.0)) if loss_weights else v
            total = term if total is None else total + term
        total.backward()
        return self._collect()

    # ---- optimiser (train_NopeSAC.py:88-169: AdamW / SGD over per-parameter groups)
    def step(self, lr: float = 1e-4, optimizer: str = "ADAMW", weight_decay: float = 0.01, betas=(0.9, 0.999), eps: float = 1e-8,
             momentum: float = 0.9, weight_decay_norm: Optional[float] = None, weight_decay_embed: Optional[float] = None):
        """`weight_decay_norm` / `weight_decay_embed` (if given): the decay of the tensors parameter_group calls "norm" / "embed" instead
        of `weight_decay` - the reference's norm and embedding parameter groups."""
        self.steps += 1
        for k, p in self.params.items():
            if p.grad is None:
                continue
            wd = self._weight_decay(k, weight_decay, weight_decay_norm, weight_decay_embed)
            g = p.grad.contiguous()
            st = self.state.setdefault(k, {})
            with torch.no_grad():
                if optimizer.upper() == "ADAMW":
                    if not st:
                        st["m1"], st["m2"] = torch.zeros_like(p), torch.zeros_like(p)
                    ops.adamw_step(p, g, st["m1"], st["m2"], lr, betas[0], betas[1], eps, wd, self.steps)
                elif optimizer.upper() == "SGD":
                    first = "mom" not in st
                    if first:
                        st["mom"] = torch.zeros_like(p)
                    ops.sgd_step(p, g, st["mom"], lr, momentum, wd, first)
                else:
                    raise NotImplementedError(f"no optimizer type {optimizer}")           # train_NopeSAC.py:158

    @staticmethod
    def _weight_decay(key: str, weight_decay: float, weight_decay_norm: Optional[float], weight_decay_embed: Optional[float] = None) -> float:
        """The decay of one tensor's optimiser group."""
        wd = {"plain": weight_decay, "norm": weight_decay_norm, "embed": weight_decay_embed}[parameter_group(key)]
        return weight_decay if wd is None else wd

    def clip_grad_norm(self, max_norm: float) -> torch.Tensor:
        """torch.nn.utils.clip_grad_norm_ over ALL parameters of this trainer (the reference's FullModelGradientClippingOptimizer,
        train_NopeSAC.py:139-148), on the device: returns the clip coefficient (f32[1]; 1 = not clipped) without a host sync."""
        grads = [p.grad for p in self.params.values() if p.grad is not None]
        acc = None
        for g in grads:
            acc = ops.sumsq_accumulate(g.contiguous(), acc)
        coef = ops.clip_coefficient(acc, max_norm)
        for p in self.params.values():
            if p.grad is not None:
                if not p.grad.is_contiguous():
                    p.grad = p.grad.contiguous()
                ops.scale_by(p.grad, coef)
        return coef

    def step_from_cfg(self, cfg):
        """One optimiser step with the reference's solver settings (Trainer.build_optimizer, train_NopeSAC.py:88-169): SOLVER.OPTIMIZER
        (ADAMW / SGD), BASE_LR, WEIGHT_DECAY, MOMENTUM, CLIP_GRADIENTS (CLIP_TYPE "full_model": global-norm clipping in front of the
        step).  Norm tensors use WEIGHT_DECAY_NORM and embeddings WEIGHT_DECAY_EMBED (parameter_group), as the reference's module types
        do; the learning rate carries `lr_multiplier(cfg)`."""
        S = cfg.SOLVER
        cg = S.CLIP_GRADIENTS
        if cg.ENABLED and cg.CLIP_TYPE == "full_model" and cg.CLIP_VALUE > 0.0:
            self.clip_grad_norm(float(cg.CLIP_VALUE))
        elif cg.ENABLED:
            raise NotImplementedError("SOLVER.CLIP_GRADIENTS.CLIP_TYPE %r (the reference's configs use full_model)" % (cg.CLIP_TYPE,))
        self.step(lr=float(S.BASE_LR) * self.lr_multiplier(cfg), optimizer=str(S.OPTIMIZER), weight_decay=float(S.WEIGHT_DECAY),
                  momentum=float(S.MOMENTUM), weight_decay_norm=float(S.WEIGHT_DECAY_NORM), weight_decay_embed=float(S.WEIGHT_DECAY_EMBED))

    def lr_multiplier(self, cfg) -> float:
        """The reference's per-module learning-rate multiplier of the module this trainer holds (train_NopeSAC.py:122-129): SOLVER's
        LR_MULTIPLIER entry, or 1.  (BACKBONE_MULTIPLIER is BackboneTrainer's; PLANE_MATCHER_HEAD_MULTIPLIER is keyed on a module name
        the reference does not have, so it never fires there either.)"""
        return 1.0 if self.LR_MULTIPLIER is None else float(getattr(cfg.SOLVER, self.LR_MULTIPLIER))


class ChainedTrainer(HeadTrainer):
    """A trainer whose output (OUTPUT: "hs", "p1" or - one trainer further up - "memory", kept by its forward in `_out`) feeds
    PlaneInstanceHeadsTrainer: its backward
    starts from the gradient the heads report there (backward_from) or, after losses(heads, ...) has put both on one graph, runs the
    heads' backward on into this trainer (backward)."""

    OUTPUT = ""

    def __init__(self, params: Dict[str, torch.Tensor]):
        super().__init__(params)
        self._out = self._heads = None

    def backward_from(self, d_out: torch.Tensor) -> Dict[str, torch.Tensor]:
        """The gradient at the last forward's output (what PlaneInstanceHeadsTrainer.input_grads[OUTPUT] holds for it) -> {state-dict
        key: gradient} of this trainer's tensors (also `.grads`); `.input_grads` = the gradients at the watched inputs."""
        _require(self._out is not None and tuple(d_out.shape) == tuple(self._out.shape),
                 "%s.backward_from: d_%s like the last forward's %s" % (type(self).__name__, self.OUTPUT, self.OUTPUT))
        self._clear_grads()
        torch.autograd.backward(self._out, d_out.contiguous())
        return self._collect()

    def backward(self, losses: Dict[str, torch.Tensor], loss_weights: Optional[Dict[str, float]] = None) -> Dict[str, torch.Tensor]:
        """The chain's backward: the instance heads' backward runs on through OUTPUT into this trainer.  -> the gradients of both trainers'
        tensors by state-dict key (the heads' own stay readable as their `.grads`; `.grads` here holds this trainer's)."""
        _require(self._heads is not None, "%s.backward: call losses() first (backward_from takes a gradient at %s)" % (type(self).__name__, self.OUTPUT))
        self._clear_grads()
        head_grads = self._heads.backward(losses, loss_weights)
        return {**self._collect(), **head_grads}


class RefineTrainer(HeadTrainer):
    """The camera head's refinement stage: forward / backward / optimiser step.

        tr = RefineTrainer.from_state_dict(sd, nq, device)             # or .from_head(model.camera_head_list[0])
        losses = tr.losses(A, planes1, planes2, n1, n2, init_trans, init_rot, init_trans_feat, init_rot_feat, gt_pose, suffix, weight)
        grads = tr.backward(losses)                                     # {state-dict key: gradient}; tr.input_grads for the feature inputs
        tr.step(lr=1e-4)                                                # AdamW (train_NopeSAC.py:150-153) on the device
        tr.write_back(head)                                             # into the inference model's packed weights
    Optimiser groups: norm / embedding groups do not occur in this head."""

    KEY_PREFIX = PREFIX

    def __init__(self, params: Dict[str, torch.Tensor], nq: int, warp_in_ref: bool = True):
        super().__init__(params)
        self.nq, self.warp_in_ref = int(nq), bool(warp_in_ref)

    @staticmethod
    def parameter_names(sd_keys) -> List[str]:
        out = []
        for k in sd_keys:
            if not k.startswith(PREFIX):
                continue
            r = k[len(PREFIX):]
            if r.split(".")[0] in MLPS + LINEARS:
                out.append(k)
        return sorted(out)

    @classmethod
    def from_state_dict(cls, sd: dict, nq: int, device, warp_in_ref: bool = True) -> "RefineTrainer":
        return cls(cls._read(sd, cls.parameter_names(sd.keys()), device), nq, warp_in_ref)

    @classmethod
    def from_head(cls, head) -> "RefineTrainer":
        return cls(cls._read(head, cls.parameter_names(cls._head_keys(head))), head.num_queries, head.warp_plane_in_cam_ref_on)

    # ---- forward
    def _mlp(self, x, name: str, final_relu: bool = False):
        return _mlp_stack(self.params, PREFIX + name, x, ops.ACT_RELU if final_relu else ops.ACT_NONE)

    def _lin(self, x, name: str, act: int = ops.ACT_NONE):
        return _linear(x, self.params[f"{PREFIX}{name}.weight"], self.params[f"{PREFIX}{name}.bias"], act)

    def losses(self, A0, planes1, planes2, n1, n2, init_trans, init_rot, init_trans_feat, init_rot_feat, gt_pose, suffix: str = "",
               weight: float = 1.0, plane_grads: bool = False) -> Dict[str, torch.Tensor]:
        """The seven losses of __forward_PlaneCamRefHead (camera_head.py:883-921) with the autograd tape attached.  The feature / pose inputs
        may require grad (their gradients land in `input_grads` after backward()).  plane_grads: planes1 / planes2 that require grad are on
        the tape as well - through the 8-d encoder input and through the hypothesis-by-plane distance maps, under the detached initial
        pose as in the reference (get_pred_geo_sequence, camera_head.py:1352-1425) - and their gradients land in `input_grads` too.  Off,
        the launches and the bits are those of the plane-free tape."""
        P, nq = self.params, self.nq
        B = A0.shape[0]
        if plane_grads:
            geo_local, geo_enc, m = _GeoSequence.apply(A0, planes1, planes2, n1, n2, init_trans.detach(), init_rot.detach(), self.warp_in_ref)
        else:
            with torch.no_grad():
                geo_local, _gg, _sig, geo_enc, m = ops.geo_sequence(A0, planes1, planes2, n1, n2, init_trans.detach(), init_rot.detach(), self.warp_in_ref)
        rows = B * nq
        geo = self._mlp(geo_enc.view(rows, 8), "geo_encoder")
        s1 = self._mlp(geo, "geo_proj_s1")
        f_rot = self._mlp(s1, "decoder_rot")
        s2 = self._mlp(torch.cat([s1, f_rot], dim=1), "geo_proj_s2")
        f_tran = self._mlp(s2, "decoder_tran")
        bc = lambda f: f.unsqueeze(1).expand(B, nq, f.shape[1]).reshape(rows, f.shape[1])
        fused_rot = self._mlp(torch.cat([bc(init_rot_feat), f_rot], dim=1), "decoder_rot2", final_relu=True)       # :980-983 (+ F.relu)
        fused_tran = self._mlp(torch.cat([bc(init_trans_feat), f_tran], dim=1), "decoder_tran2", final_relu=True)
        rot_raw = self._lin(fused_rot, "rots").view(B, nq, 4)
        trans_raw = self._lin(fused_tran, "trans").view(B, nq, 3)
        ns, ps, l2, rots_all, trans_all, dn_sum, dl2_sum = _ScoreMaps.apply(geo_local, rot_raw, trans_raw, init_rot, init_trans, m)
        NH = nq + 1
        sf_rot = self._mlp(ns.view(B * NH, nq), "normal_score_proj").view(B, NH, 64)
        sf_tran = self._mlp(ps.view(B * NH, nq), "param_score_proj").view(B, NH, 64)
        w = lambda n: P[f"{PREFIX}{n}.weight"]
        bb = lambda n: P[f"{PREFIX}{n}.bias"]
        pr, pt, ar, at, sr, st = _Vote.apply(sf_rot, sf_tran, w("rot_score_reg").view(-1), bb("rot_score_reg"), w("trans_score_reg").view(-1),
                                             bb("trans_score_reg"), init_rot_feat, init_trans_feat, fused_rot.view(B, nq, 256),
                                             fused_tran.view(B, nq, 256), w("rots"), bb("rots"), w("trans"), bb("trans"), rots_all, trans_all,
                                             dn_sum, dl2_sum, init_rot.detach(), init_trans.detach(), m)
        lv = _Losses.apply(pr, pt, ar, at, sr, st, l2, rots_all, trans_all, m, gt_pose, float(weight))
        watched = {"init_trans_feat": init_trans_feat, "init_rot_feat": init_rot_feat, "init_trans": init_trans, "init_rot": init_rot}
        if plane_grads:
            watched.update(planes1=planes1, planes2=planes2)
        self._watch(watched)
        self.last = {"pred_rot": pr, "pred_trans": pt, "avg_rot": ar, "avg_trans": at, "score_rot": sr, "score_trans": st, "m": m}
        return {"%s_%s" % (nm, suffix): lv[i] for i, nm in enumerate(ops.PLANE_CAM_REF_LOSS_NAMES)}


class CameraHeadTrainer(RefineTrainer):
    """The camera head in TRAINING mode (reference PlaneCameraHead.forward, camera_head.py:140-344) with every Linear layer trainable:
    the pixel pose net's FC layers + pose regressors (fc_trans / fc_rots / trans / rots), the AIM (rot_emb_proj / trans_emb_proj) and the
    refinement head - 108 tensors.  By default the pixel pose net's CONVOLUTIONS (pixel decoder, correlation stack) are frozen: their
    output features [B, 768] are computed by the inference kernels and enter as constants (`conv_feats`).

    conv_stacks=True trains them too (179 tensors: + 24 conv weights, mask_features.bias, 10 GroupNorm and 36 BatchNorm affine tensors,
    the reference's step-2 / step-3 recipe): the pixel pose net runs in f32 from this trainer's parameters on the 2B images (view 1
    first, siamese weights shared) and its backward is csrc/conv_bwd.hip.  By default BatchNorm uses the stored running statistics
    (buffers, never updated) with a trainable affine.  feature_grads=True also returns the gradients of the backbone maps in
    `input_grads["res3" / "res4" / "res5"]` (NHWC, [2B, h, w, C]).

    batch_stats=True (needs conv_stacks=True) trains the 18 conv + BatchNorm + LeakyReLU blocks as the reference does, which never freezes
    them (MODEL.FREEZE = []): every BatchNorm normalises by the batch's own mean and variance and is differentiated through them
    (csrc/camera_bn_train.hip).  The siamese tower convs_backbone runs once per view in the reference (camera_head.py:646-647): its
    statistics are taken over view 1's B images and over view 2's B images separately (groups = 2 over the 2B-image batch), its running
    buffers are updated twice per iteration in that order and its counters advance by 2; the two branches see the B pairs once
    (groups = 1, counters + 1).  `buffers` then holds clones of the 36 running statistics (f32, updated in place on the device; momentum
    0.01, unbiased variance) and the 18 num_batches_tracked counters (int64); one camera_head_losses call is one training iteration, and
    write_back copies the buffers into the inference head too.  `tr.batch_stats = False` between steps runs the stored-statistics path
    on the trainer's current buffers (validation) and leaves them untouched.
    Detach points as in the reference: the AIM re-embeds a detached copy of the pixel pose (:694, :723); the geometry sequences are built
    from detached initial poses (:354-365)."""

    EXTRA_MLPS = ("rot_emb_proj", "trans_emb_proj")
    EXTRA_LINEARS = ("fc_trans", "fc_rots")

    def __init__(self, params: Dict[str, torch.Tensor], nq: int, warp_in_ref: bool = True, buffers: Optional[Dict[str, torch.Tensor]] = None,
                 conv_stacks: bool = False, feature_grads: bool = False, batch_stats: bool = False):
        super().__init__(params, nq, warp_in_ref)
        self.conv_stacks, self.feature_grads, self.batch_stats = bool(conv_stacks), bool(feature_grads), bool(batch_stats)
        _require(not self.feature_grads or self.conv_stacks, "feature_grads needs conv_stacks=True")
        _require(not self.batch_stats or self.conv_stacks, "batch_stats needs conv_stacks=True")
        if self.batch_stats:                                      # the trainer's own copies: a forward updates them in place
            self.buffers = {k: (v.detach().clone().to(torch.int64) if k.endswith("num_batches_tracked") else v.detach().clone().float().contiguous())
                            for k, v in (buffers or {}).items()}
            _require(len(self.buffers) == 54, "batch_stats=True: 36 running statistics and 18 counters expected, got %d buffers" % len(self.buffers))
        else:
            self.buffers = {k: v.detach().float().contiguous() for k, v in (buffers or {}).items()}
        if self.conv_stacks:
            missing = [k for k in self.parameter_names(list(self.params) + list(self.buffers), True) if k not in self.params]
            _require(not missing, "conv_stacks=True: missing parameters %s" % (missing,))

    @staticmethod
    def parameter_names(sd_keys, conv_stacks: bool = False) -> List[str]:
        out = []
        groups = MLPS + LINEARS + CameraHeadTrainer.EXTRA_MLPS + CameraHeadTrainer.EXTRA_LINEARS + (CONV_STACKS if conv_stacks else ())
        for k in sd_keys:
            if not k.startswith(PREFIX) or k.split(".")[-1] in _BUFFER_LEAVES:
                continue
            if k[len(PREFIX):].split(".")[0] in groups:
                out.append(k)
        return sorted(out)

    @staticmethod
    def buffer_names(sd_keys, counters: bool = False) -> List[str]:
        """The BatchNorm running statistics of the conv stacks (fixed inputs of the stored-statistics forward; updated by a
        batch-statistics one), with `counters` also their num_batches_tracked."""
        leaves = _BUFFER_LEAVES if counters else ("running_mean", "running_var")
        return sorted(k for k in sd_keys if k.startswith(PREFIX) and k[len(PREFIX):].split(".")[0] in CONV_STACKS
                      and k.split(".")[-1] in leaves)

    @classmethod
    def from_state_dict(cls, sd: dict, nq: int, device, warp_in_ref: bool = True, conv_stacks: bool = False,
                        feature_grads: bool = False, batch_stats: bool = False) -> "CameraHeadTrainer":
        return cls(cls._read(sd, cls.parameter_names(sd.keys(), conv_stacks), device), nq, warp_in_ref,
                   cls._read(sd, cls.buffer_names(sd.keys(), batch_stats), device) if conv_stacks else None, conv_stacks, feature_grads,
                   batch_stats)

    @classmethod
    def from_head(cls, head, conv_stacks: bool = False, feature_grads: bool = False, batch_stats: bool = False) -> "CameraHeadTrainer":
        keys = cls._head_keys(head)
        return cls(cls._read(head, cls.parameter_names(keys, conv_stacks)), head.num_queries, head.warp_plane_in_cam_ref_on,
                   cls._read(head, cls.buffer_names(keys, batch_stats)) if conv_stacks else None, conv_stacks, feature_grads, batch_stats)

    def _written_back(self) -> Dict[str, torch.Tensor]:
        """write_back copies the trained parameters; a trainer built with batch_stats=True also its running statistics and counters (the
        head's BatchNorm folds are dropped with its other packed copies and rebuilt on the next forward)."""
        counted = any(k.endswith("num_batches_tracked") for k in self.buffers)
        return {**self.params, **self.buffers} if counted else self.params

    # ---- the pixel pose net's conv stacks (conv_stacks=True), camera_head.py:642-667 / camera_modules.py:246-348
    def _cbl(self, x, name: str, stride: int = 1):
        """conv3x3 (no bias) + BatchNorm2d(eps 1e-3, momentum 0.01) + LeakyReLU(0.01) (camera_modules.py:36-48): on the stored statistics,
        or with batch_stats on the batch's (per view in the siamese tower), the running buffers and the counter updated in place."""
        P, Bf = self.params, self.buffers
        q = PREFIX + name
        if self.batch_stats:
            groups = 2 if name.startswith("convs_backbone.") else 1
            _require(q + ".1.num_batches_tracked" in Bf, "batch_stats: this trainer was built without the BatchNorm counters (batch_stats=True)")
            y = _ConvBNActBatch.apply(x, P[q + ".0.weight"], P[q + ".1.weight"], P[q + ".1.bias"], Bf[q + ".1.running_mean"],
                                      Bf[q + ".1.running_var"], stride, 1, groups)
            Bf[q + ".1.num_batches_tracked"] += groups
            return y
        return _ConvBNAct.apply(x, P[q + ".0.weight"], P[q + ".1.weight"], P[q + ".1.bias"], Bf[q + ".1.running_mean"],
                                Bf[q + ".1.running_var"], stride, 1, ops.ACT_LEAKY)

    def _gn_conv(self, x, name: str, pad: int, relu: bool):
        q = PREFIX + "pixel_decoder." + name
        return _ConvGN.apply(x, self.params[q + ".weight"], self.params[q + ".norm.weight"], self.params[q + ".norm.bias"], pad, relu)

    def pixel_pose_convs(self, feats: dict, B: int):
        """The conv stacks on NHWC res3..res5 of 2B images (view 1 first) -> yt, yr [B, 768] in the reference's flatten order, with the
        autograd tape attached."""
        y = self._gn_conv(feats["res5"], "layer_3", 1, True)
        y = _UpsampleAdd.apply(y, self._gn_conv(feats["res4"], "adapter_2", 0, False))
        y = self._gn_conv(y, "layer_2", 1, True)
        y = _UpsampleAdd.apply(y, self._gn_conv(feats["res3"], "adapter_1", 0, False))
        y = self._gn_conv(y, "layer_1", 1, True)
        q = PREFIX + "pixel_decoder.mask_features"
        x = _ConvBias.apply(y, self.params[q + ".weight"], self.params[q + ".bias"], 1)
        for i in BACKBONE_CONVS:
            x = self._cbl(x, f"convs_backbone.{i}")
            if i in (1, 4):
                x = _MaxPool2.apply(x)
        _, h, w, _ = x.shape
        P = h * w
        aff = _CorrSoftmax.apply(x[:B], x[B:], P + (-P) % 8)          # (300 -> 304 channels at 480 x 640, zeros beyond P)

        def branch(name):
            t = aff
            for i in range(6):
                t = self._cbl(t, f"{name}.{i}", 2 if i % 2 == 1 else 1)
            Bt, th, tw, C = t.shape
            return t.reshape(Bt, th * tw, C).transpose(1, 2).reshape(Bt, C * th * tw)       # NHWC -> the reference's c * hw + i order

        return branch("convs_trans"), branch("convs_rots")

    def pixel_pose(self, yt: torch.Tensor, yr: torch.Tensor):
        """The FC layers + regressors on the conv features yt / yr [B, 768] in the REFERENCE's flatten order (channel-major: c * 6 + hw)."""
        trans_feat = self._lin(yt, "fc_trans", ops.ACT_RELU)
        rots_feat = self._lin(yr, "fc_rots", ops.ACT_RELU)
        trans0 = self._lin(trans_feat, "trans")
        rot0 = _Normalize.apply(self._lin(rots_feat, "rots"), False)
        return trans0, rot0, trans_feat, rots_feat

    def aim(self, trans_in: torch.Tensor, rot_in: torch.Tensor):
        """__forward_RotRecHead / __forward_TransRecHead (:685-735) on DETACHED inputs; returns (rec_trans, rec_rot, trans_feat, rot_feat,
        the canonical-sign input rotation, the shifted input translation)."""
        rot_c = ops.normalize_rows(rot_in.detach().contiguous(), canonical_sign=True)
        tr_in = (trans_in.detach() + 1e-10).contiguous()
        rot_feat = self._mlp(rot_c, "rot_emb_proj", final_relu=True)
        rec_rot = _Normalize.apply(self._lin(rot_feat, "rots"), False)
        trans_feat = self._mlp(tr_in, "trans_emb_proj", final_relu=True)
        rec_trans = self._lin(trans_feat, "trans")
        return rec_trans, rec_rot, trans_feat, rot_feat, rot_c, tr_in

    def camera_head_losses(self, head, feats: dict, B: int, gt_planes1, gt_planes2, gt_n1, gt_n2, gt_assignment, gt_pose, planes1=None, planes2=None,
                           n1=None, n2=None, assignment=None, rand_rot=None, rand_trans=None, plane_grads: bool = False) -> Dict[str, torch.Tensor]:
        """All losses of the training-mode forward (the 34 of PlaneCameraHead.forward_train) with the autograd tape attached.  plane_grads
        puts the PREDICTED planes of the _Aux passes on the tape (RefineTrainer.losses; their gradients land in `input_grads` under
        planes1 / planes2); the ground-truth planes are data."""
        inputs = {}
        if self.conv_stacks:
            fm = {}
            for k in ("res3", "res4", "res5"):
                fm[k] = feats[k].detach().float().contiguous()
                if self.feature_grads:
                    fm[k].requires_grad_(True)
                    inputs[k] = fm[k]
            yt, yr = self.pixel_pose_convs(fm, B)
            yt, yr = yt.contiguous(), yr.contiguous()
            self.conv_feats = (yt.detach(), yr.detach())
        else:
            with torch.no_grad():
                yt, yr = head.pixel_pose_net(feats, B, features_only=True)          # [B, hw * 128 + c]: the inference kernels' NHWC order
                to_ref = lambda y: y.view(B, 6, 128).transpose(1, 2).reshape(B, 768).contiguous().float()
                yt, yr = to_ref(yt), to_ref(yr)
            self.conv_feats = (yt, yr)                            # (what the frozen conv stacks handed to the trainable layers)
        losses: Dict[str, torch.Tensor] = {}
        trans0, rot0, tf0, rf0 = self.pixel_pose(yt, yr)
        lp = _PoseLoss.apply(trans0, rot0, gt_pose[:, 0:3], gt_pose[:, 3:7], head.initial_cam_weight, 0.0)
        losses["loss_tran_pixelReg"], losses["loss_rot_pixelReg"] = lp[0], lp[1]

        def rec(trans_in, rot_in, suffix):
            rec_t, rec_r, rec_tf, rec_rf, rot_c, tr_in = self.aim(trans_in, rot_in)
            lr = _PoseLoss.apply(rec_t, rec_r, tr_in, rot_c, 1.0, 0.0)           # (tr_in already carries the + 1e-10)
            losses["loss_rot" + suffix], losses["loss_trans" + suffix] = lr[1], lr[0]
            return rec_t, rec_r, rec_tf, rec_rf

        rec_t, rec_r, rec_tf, rec_rf = rec(trans0, rot0, "_initCamRec")
        passes = [("", gt_planes1, gt_planes2, gt_n1, gt_n2, gt_assignment, head.plane_cam_weight, False)]
        if assignment is not None:
            passes.append(("_Aux", planes1, planes2, n1, n2, assignment, head.plane_cam_weight_predplane, bool(plane_grads)))
            if plane_grads:
                inputs.update(planes1=planes1, planes2=planes2)
        self.recorded = {"trans": [trans0, rec_t], "rot": [rot0, rec_r]}
        for sfx, pl1, pl2, c1, c2, A, w, pg in passes:
            for name, it, ir, itf, irf in (("initCamRef", trans0, rot0, tf0, rf0), ("initRecCamRef", rec_t, rec_r, rec_tf, rec_rf)):
                losses.update(self.losses(A, pl1, pl2, c1, c2, it, ir, itf, irf, gt_pose, suffix=name + sfx, weight=w, plane_grads=pg))
                self.recorded["trans"] += [self.last["avg_trans"], self.last["pred_trans"]]
                self.recorded["rot"] += [self.last["avg_rot"], self.last["pred_rot"]]
        if rand_rot is not None:
            rec(rand_trans, rand_rot, "_randCamRecLBS_N1")
        self._watch(inputs)                                       # (the backbone maps, in place of what the last losses() call watched)
        return losses


class MatchingHeadTrainer(HeadTrainer):
    """The matching head in TRAINING mode (reference MatchingHead.forward + embedding_loss_forward, matching_net/matching_head.py:43-139;
    LoFTR-style GNN, transformer/gnn.py:73-134): every floating tensor under `matching_head.` is trainable - 185 tensors: 18 layers x
    (q_proj, k_proj, v_proj, merge, mlp.0, mlp.2, norm1 weight / bias, norm2 weight / bias), planeApp_proj and planeDesc_proj weight / bias
    and bin_score.

        tr = MatchingHeadTrainer.from_state_dict(sd, nq, device)        # or .from_head(model.matching_head)
        losses = tr.matching_losses(app, n_all, cam7, planes1, planes2, gt_corr, suffix)
        grads = tr.backward(losses); tr.step(lr=1e-4); tr.write_back(model.matching_head)

    Ragged plane sets are padded to nq rows with int32 lengths, as everywhere in this code base.  The reference's masked subsets of
    queries (`indices1` / `indices2`, matching_head.py:51-69) are passed COMPACTED to a prefix: a masked row gets zero weight in the
    attention (gnn.py masks) and -1e5 in the Sinkhorn, and its gt_corr entries are cleared by the logical_and of :69 - exactly what a row
    beyond the length is here - so the caller gathers the selected queries (and the matching rows / columns of gt_corr) to the front.

    Optimiser groups (train_NopeSAC.py:88-135): the 72 LayerNorm tensors take WEIGHT_DECAY_NORM (parameter_group), bin_score and every
    other tensor the plain WEIGHT_DECAY.  SOLVER.PLANE_MATCHER_HEAD_MULTIPLIER is NOT applied: the reference keys it on
    "plane_matcher_net" in module_name, the module is called `matching_head`, so it never fires there either."""

    KEY_PREFIX = MATCHER_PREFIX

    def __init__(self, params: Dict[str, torch.Tensor], nq: int, offset_multiplier: float = 4.0, normal_multiplier: float = 8.0,
                 sinkhorn_iterations: int = 200):
        super().__init__(params)
        self.nq = int(nq)
        self.offset_multiplier, self.normal_multiplier = float(offset_multiplier), float(normal_multiplier)
        self.sinkhorn_iterations = int(sinkhorn_iterations)                       # matching_head.py:38

    @staticmethod
    def parameter_names(sd_keys) -> List[str]:
        return sorted(k for k in sd_keys if k.startswith(MATCHER_PREFIX) and k.split(".")[-1] not in _BUFFER_LEAVES)

    @classmethod
    def from_state_dict(cls, sd: dict, nq: int, device, **kw) -> "MatchingHeadTrainer":
        names = [k for k in cls.parameter_names(sd.keys()) if torch.is_tensor(sd[k]) and sd[k].is_floating_point()]
        return cls(cls._read(sd, names, device), nq, **kw)

    @classmethod
    def from_head(cls, head) -> "MatchingHeadTrainer":
        return cls(cls._read(head, cls.parameter_names(cls._head_keys(head))), head.num_queries, head.offset_multiplier, head.normal_multiplier,
                   head.sinkhorn_iterations)

    # ---- forward
    def _gnn_layer(self, i: int, x, src, nb: int, qlen, klen):
        """x + LN2(mlp(cat[x, LN1(merge(attention(q(x), k(src), v(src))))])) (gnn.py:73-96) with the GEMMs grouped exactly as
        MatchingHead._gnn_layer groups them on its f32 route - one q|k|v projection in a self layer, q and k|v in a cross layer, mlp.0 as
        two products - so that the same parameters give the inference head's values bit for bit.  The concatenated weights are autograd
        views of the per-tensor leaves: their gradients come back as row slices."""
        P, nq, p = self.params, self.nq, f"{MATCHER_PREFIX}gnn.layers.{i}"
        w = lambda name: P[f"{p}.{name}.weight"]
        scale = 32 ** -0.5
        if x is src:
            qkv = _linear(x, torch.cat([w("q_proj"), w("k_proj"), w("v_proj")], 0))
            msg = _AttentionFused.apply(None, qkv, nb, nq, nq, GNN_HEADS, scale, qlen, klen)
        else:
            q = _linear(x, w("q_proj"))
            kv = _linear(src, torch.cat([w("k_proj"), w("v_proj")], 0))
            msg = _AttentionFused.apply(q, kv, nb, nq, nq, GNN_HEADS, scale, qlen, klen)
        msg = _LayerNorm.apply(_linear(msg, w("merge")), P[p + ".norm1.weight"], P[p + ".norm1.bias"], None)
        out = _linear(_LinearSplit.apply(x, msg, w("mlp.0")), w("mlp.2"))
        return _LayerNorm.apply(out, P[p + ".norm2.weight"], P[p + ".norm2.bias"], x)

    def matching_losses(self, app, n_all, cam7, planes1, planes2, gt_corr, suffix: str = "",
                        iterations: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """app [2B, nq, 256] (view-1 sets first), n_all int32[2B], cam7 [B, 7] = (t, q), planes1 / planes2 [B, nq, 3], gt_corr uint8 / bool
        [B, nq+1, nq+1] (dustbin at index nq; entries outside a pair's live block are ignored) -> {"losses_emb_<suffix>": scalar} with
        the autograd tape attached; `last["log_scores_padded"]` keeps the Sinkhorn output.  `app` may require grad (its gradient lands in
        `input_grads["app"]`, zero in padded rows).  A batch whose gt_corr selects nothing gives loss 0 and zero gradients (the reference
        returns NaN there)."""
        P, nq = self.params, self.nq
        B = cam7.shape[0]
        rows = B * nq
        iters = self.sinkhorn_iterations if iterations is None else int(iterations)
        n_all = n_all.contiguous()
        n1, n2 = n_all[:B].contiguous(), n_all[B:].contiguous()
        gt = gt_corr.to(torch.uint8).contiguous()
        _require(app.shape == (2 * B, nq, 256) and gt.shape == (B, nq + 1, nq + 1) and n_all.dtype == torch.int32,
                 "matching_losses: app [2B,nq,256], gt_corr [B,nq+1,nq+1], n_all int32; got %s, %s, %s" % (tuple(app.shape), tuple(gt.shape), n_all.dtype))
        q = MATCHER_PREFIX
        f = _linear(app.reshape(2 * rows, 256), P[q + "planeApp_proj.weight"].view(256, 256), P[q + "planeApp_proj.bias"])
        for i in range(GNN_LAYERS):
            if i % 2 == 0:                       # 'self' (gnn.py:128-130): both sets in one call
                f = self._gnn_layer(i, f, f, 2 * B, n_all, n_all)
            else:                                # 'cross' (gnn.py:131-133): feat1 attends to the UPDATED feat0
                f0 = self._gnn_layer(i, f[:rows], f[rows:], B, n1, n2)
                f1 = self._gnn_layer(i, f[rows:], f0, B, n2, n1)
                f = torch.cat([f0, f1], 0)
        d = _linear(f, P[q + "planeDesc_proj.weight"].view(256, 256), P[q + "planeDesc_proj.bias"])
        dots = _DescDot.apply(d[:rows].view(B, nq, 256), d[rows:].view(B, nq, 256), n1, n2)
        loss, log_scores = _SinkhornEmbLoss.apply(dots, P[q + "bin_score"].view(1), planes1.contiguous(), planes2.contiguous(), cam7.contiguous(),
                                                  n1, n2, gt, self.offset_multiplier, self.normal_multiplier, iters)
        self._watch({"app": app})
        self.last = {"log_scores_padded": log_scores, "desc_dot": dots.detach()}
        return {"losses_emb_%s" % suffix: loss}


# ---- the plane head's set criterion ------------------------------------------------------------------------------------------------------
PLANE_LAYER_LOSSES = ("loss_ce", "loss_mask", "loss_dice", "loss_center_ins", "loss_param_l1", "loss_param_cos")
PLANE_LAST_LOSSES = ("loss_center_pixel", "loss_q")


class _PlaneLosses(torch.autograd.Function):
    """ops.plane_losses / ops.plane_losses_backward on a PlaneCriterionCall whose match is already made: (pred_logits, pred_mask_logits,
    pred_centers, pred_params [L*B, ...], pixel_centers or None) -> losses [6 L + 2], or [G, 6 L + 2] of a grouped call.  Bookkeeping only."""

    @staticmethod
    def forward(ctx, call, logits, mask_logits, centers, params, pixel_centers):
        ctx.call = call
        return ops.plane_losses(call).clone()

    @staticmethod
    def backward(ctx, g):
        d_lg, d_ml, d_ce, d_pa, d_px = ops.plane_losses_backward(ctx.call, g.contiguous().float())
        return None, d_lg, d_ml, d_ce, d_pa, d_px


class PlaneCriterion:
    """HungarianMatcher + SetCriterion of the plane head on the device.  criterion(outputs, targets) -> (losses, indices):
    outputs = the reference's dict - pred_logits [B, nq, 2], pred_mask_logits [B, nq, h, w] (any dense stride order: the head's
    [B, h, w, nq] tensor goes in as .permute(0, 3, 1, 2) without a copy), pred_centers [B, nq, 2], pred_params [B, nq, 3], pixel_centers
    [B, 2, h, w] (likewise) and aux_outputs = a list of dicts with the first four;
    targets = masks uint8 [B, nmax, H, W], n (int32 on the host, or a list: the planes per image, 1..min(nq, 50)), plane_params [B, nmax, 3],
    depth [B, H, W], k_inv_dot_xy1 [B, 3, H, W];
    losses = the reference's names (aux layers with _0, _1, ...), unweighted, attached to autograd; weighted(losses) applies weight_dict
    as forward_single does; indices = {"match_q" int32 [L, B, nmax], "match_gt" int32 [L, B, nq], "n"} on the device, layer 0 = the last
    decoder layer.  The reference's all-reduce of num_masks over ranks is the caller's: pass the reduced value as num_masks.

    groups = G: the batch is G groups of B / G consecutive images (the two views of a 2B-image pass: groups=2), and every batch-wide
    normaliser - num_masks, the matched count, the class weight sum, the B of loss_center_pixel and loss_q - is the group's, as the
    reference's forward_single per view has them (siamese_planeTR.py:228-235).  Each returned loss is ((l_0 + l_1) + ...) / G over the
    per-group values, summed in group order - the reference's (losses1[k] + losses2[k]) / 2 - and last["group_losses"] keeps the
    per-group dicts (on the tape: a caller that weighs before it averages, as forward_single does, takes them).  num_masks: one value for every group, or G values.  groups=1 is the ungrouped call, bit for bit."""

    def __init__(self, cost_class=1.0, cost_mask=20.0, cost_dice=1.0, cost_center=0.5, cost_param=0.5, cost_offset=0.01, cost_angle=0.0028,
                 eos_coef=0.1, weight_dict: Optional[Dict[str, float]] = None, num_classes: int = 1):
        self.weights = dict(cost_class=cost_class, cost_mask=cost_mask, cost_dice=cost_dice, cost_center=cost_center, cost_param=cost_param,
                            cost_offset=cost_offset, cost_angle=cost_angle, eos_coef=eos_coef)
        self.weight_dict = dict(weight_dict or {})
        self.num_classes = int(num_classes)

    @classmethod
    def from_cfg(cls, cfg):
        """The weights of from_config (siamese_planeTR.py:136-185)."""
        H = cfg.MODEL.SEM_SEG_HEAD
        wd = {"loss_ce": 1, "loss_param_l1": H.PARAM_WEIGHT_L1, "loss_param_cos": H.PARAM_WEIGHT_COS, "loss_q": H.PARAM_WEIGHT_Q,
              "loss_center_ins": H.PARAM_WEIGHT_CENTER_INS, "loss_center_pixel": 1.0, "loss_depth_pixel": 1.0, "loss_mask": H.MASK_WEIGHT,
              "loss_dice": H.DICE_WEIGHT}
        if H.DEEP_SUPERVISION:
            aux = {}
            for i in range(H.DEC_LAYERS - 1):
                aux.update({k + f"_{i}": v for k, v in wd.items()})
            wd.update(aux)
        return cls(cost_class=1, cost_mask=H.MASK_WEIGHT, cost_dice=H.DICE_WEIGHT, cost_center=H.PARAM_WEIGHT_CENTER_INS,
                   cost_param=H.PARAM_HM_WEIGHT_L1, cost_offset=H.PARAM_WEIGHT_OFFSET, cost_angle=H.PARAM_WEIGHT_ANGLE,
                   eos_coef=H.NO_OBJECT_WEIGHT, weight_dict=wd, num_classes=H.NUM_CLASSES)

    def prepare_targets(self, targets: dict) -> dict:
        """Adds n (device) / n_host, plane_centers and pixel_centers (prepare_targets, siamese_planeTR.py:498-504) unless they are there."""
        t = dict(targets)
        dev = t["masks"].device
        n = t["n_host"] if "n_host" in t else t["n"]
        n_host = torch.as_tensor(n, dtype=torch.int32).cpu().contiguous()
        t["n_host"] = n_host
        if not (torch.is_tensor(t.get("n")) and t["n"].is_cuda and t["n"].dtype == torch.int32):
            t["n"] = n_host.to(dev)
        t["masks"] = t["masks"].contiguous()
        for k in ("plane_params", "depth", "k_inv_dot_xy1"):
            t[k] = t[k].float().contiguous()
        if "plane_centers" not in t or "pixel_centers" not in t:
            t["plane_centers"], t["pixel_centers"] = ops.plane_targets(t["masks"], n_host, t["n"])
        return t

    def __call__(self, outputs: dict, targets: dict, num_masks=None, groups: int = 1):
        layers = [outputs] + list(outputs.get("aux_outputs", []))
        L = len(layers)
        B, nq = outputs["pred_logits"].shape[:2]
        G = int(groups)
        _require(G >= 1 and B % G == 0, "PlaneCriterion: groups=%d does not divide the batch of %d" % (G, B))
        t = self.prepare_targets(targets)
        if L == 1:
            ml = outputs["pred_mask_logits"]
            if torch.empty_like(ml).stride() != ml.stride():
                ml = ml.contiguous()
            stack = lambda k: outputs[k].contiguous()
        else:
            ml = torch.stack([o["pred_mask_logits"] for o in layers]).flatten(0, 1)
            stack = lambda k: torch.stack([o[k] for o in layers]).flatten(0, 1)
        px = outputs.get("pixel_centers")
        if px is not None and torch.empty_like(px).stride() != px.stride():
            px = px.contiguous()
        preds = {"pred_logits": stack("pred_logits"), "pred_mask_logits": ml, "pred_centers": stack("pred_centers"),
                 "pred_params": stack("pred_params"), "pixel_centers": px}
        call = ops.PlaneCriterionCall(L, {k: (None if v is None else v.detach()) for k, v in preds.items()}, t, self.weights,
                                      0.0 if num_masks is None else num_masks, G)
        ops.plane_match_costs(call)
        ops.plane_assign(call)
        vec = _PlaneLosses.apply(call, preds["pred_logits"], ml, preds["pred_centers"], preds["pred_params"], px)

        def named(v):
            out = {}
            for l in range(L):
                sfx = "" if l == 0 else "_%d" % (l - 1)
                for k, name in enumerate(PLANE_LAYER_LOSSES):
                    out[name + sfx] = v[6 * l + k]
            if px is not None:
                out["loss_center_pixel"] = v[6 * L]
            out["loss_q"] = v[6 * L + 1]
            return out
        nmax = t["masks"].shape[1]
        self.last = {"cost": call.cost.view(L, B, nq, nmax), "targets": t}
        if G == 1:
            losses = named(vec)
            self.last["group_losses"] = [dict(losses)]
        else:
            mean = vec[0]
            for g in range(1, G):                                                # in group order: (l_0 + l_1) / 2 for the two views
                mean = mean + vec[g]
            losses = named(mean / G)
            self.last["group_losses"] = [named(vec[g]) for g in range(G)]
        return losses, {"match_q": call.match_q.view(L, B, nmax), "match_gt": call.match_gt.view(L, B, nq), "n": t["n_host"].tolist()}

    def weighted(self, losses: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """forward_single's weighting (siamese_planeTR.py:329-334): losses without an entry in weight_dict are dropped."""
        return {k: v * self.weight_dict[k] for k, v in losses.items() if k in self.weight_dict}

    @staticmethod
    def indices_as_reference(indices: dict, layer: int = 0):
        """The reference's form of one layer's match: per image (src sorted ascending, tgt) int64 pairs (a host copy)."""
        mq = indices["match_q"][layer].cpu().long()
        out = []
        for b, nb in enumerate(indices["n"]):
            src, order = torch.sort(mq[b, :nb])
            out.append((src, order))
        return out


# ---- the plane head's instance heads -----------------------------------------------------------------------------------------------------
PLANE_INSTANCE_HEADS = ("plane_embedding", "pixel_embedding", "plane_prob", "plane_param", "plane_center", "pixel_plane_center")
FOLD_WIDTH = 264                       # the folded mask operand's row: 256 mask weights | the mask bias | 7 zero columns (PlaneTRHead.pack)


class _MaskProduct(torch.autograd.Function):
    """(fold [L*B*nq, 264] = mask weights | mask bias | pad, rows in (l, b, q) order; p1 [B, h, w, 256]; the pixel-centre conv's weight
    [2, 256, 1, 1] and bias) -> (mask logits [L, B, nq, h, w], pixel centres [B, 2, h, w]).  Forward: per layer the batched-weights f32
    conv the inference head launches (PlaneTRHead._heads) and its 256 -> 2 sigmoid conv; the NHWC results are stacked into the
    pixel-minor layout the criterion works in.  Backward: ops.mask_product_backward - one wgrad and one dgrad launch of
    csrc/plane_head_bwd.hip, the centre conv joined to both as two more rows, so p1's gradient is written once."""

    @staticmethod
    def forward(ctx, fold, p1, wc, bc, L: int, B: int, nq: int):
        fold = fold.contiguous()
        per = []
        for l in range(L):
            blk = fold[l * B * nq:(l + 1) * B * nq]
            mw = blk[:, :256].contiguous().view(B, nq, 1, 1, 256)
            mb = blk[:, 256].contiguous().view(B, nq)
            per.append(ops.conv2d(p1, mw, None, mb, batched_weights=True, out_dtype=torch.float32).permute(0, 3, 1, 2))
        masks = torch.stack(per)
        pc = ops.conv2d(p1, _ohwi(wc, 256), None, bc.detach().contiguous(), act=ops.ACT_SIGMOID, out_dtype=torch.float32)
        pc = pc.permute(0, 3, 1, 2).contiguous()
        ctx.dims = (L, B, nq, p1.shape[1], p1.shape[2])
        ctx.save_for_backward(fold, p1, wc, pc)
        return masks, pc

    @staticmethod
    def backward(ctx, g_masks, g_pc):
        fold, p1, wc, pc = ctx.saved_tensors
        L, B, nq, h, w = ctx.dims
        g_masks = torch.zeros(L, B, nq, h, w, device=p1.device) if g_masks is None else g_masks.contiguous()
        dz = ops.sigmoid_backward(torch.zeros_like(pc) if g_pc is None else g_pc.contiguous(), pc)
        g_fold = torch.zeros_like(fold)
        _, _, d_p1, d_wc, d_bc = ops.mask_product_backward(g_masks, fold[:, :256], p1, dz, wc.detach().view(2, 256), d_fold=g_fold[:, :256],
                                                           d_beta=g_fold[:, 256], which="both" if ctx.needs_input_grad[1] else "wgrad")
        return g_fold, d_p1, d_wc.view_as(wc), d_bc, None, None, None


class PlaneInstanceHeadsTrainer(HeadTrainer):
    """The plane head's instance heads in TRAINING mode (reference PlaneTRHead.forward, planeTR_head.py:146-192, under deep supervision):
    the 24 tensors of plane_embedding, pixel_embedding, plane_prob, plane_param, plane_center and pixel_plane_center, held under their
    state-dict keys (`sem_seg_head. ...`).  The head's trunk is frozen: its two outputs enter as inputs.

        hs, p1 = model.sem_seg_head.training_inputs(features)           # [L, B, nq, 256], [B, h, w, 256] (no autograd)
        tr = PlaneInstanceHeadsTrainer.from_head(model.sem_seg_head)    # or .from_state_dict(sd, nq, device)
        losses, indices = tr.losses(hs, p1, targets)                    # PlaneCriterion.from_cfg on the deep-supervision outputs
        grads = tr.backward(losses)                                     # the criterion's weights; tr.input_grads["hs" / "p1"] on request
        tr.step_from_cfg(cfg); tr.write_back(model.sem_seg_head)

    The mask logits are evaluated in the folded form of the inference head, M = (E W_pe) . p1 + E . b_pe: W_pe^T and b_pe enter the fold's
    Linear as autograd views of the two pixel_embedding leaves, so their gradients come back as slices of one wgrad.  Every launch of
    the last layer is the launch PlaneTRHead.forward makes on its f32 route, so the same parameters give the same bits.
    Optimiser groups (train_NopeSAC.py:88-135): none of the 24 tensors is a norm or an embedding parameter; the learning rate carries
    SOLVER.SEM_SEG_HEAD_MULTIPLIER (train_NopeSAC.py:126-127).  write_back drops the head's pe_fold, which is derived from pixel_embedding,
    with its other packed copies."""

    KEY_PREFIX, LR_MULTIPLIER = PLANE_PREFIX, "SEM_SEG_HEAD_MULTIPLIER"

    def __init__(self, params: Dict[str, torch.Tensor], nq: int, cfg=None):
        super().__init__(params)
        self.nq = int(nq)
        if cfg is None:
            from .config import get_cfg
            cfg = get_cfg()
        self.criterion = PlaneCriterion.from_cfg(cfg)
        _require(len(self.params) == 24, "PlaneInstanceHeadsTrainer: 24 tensors expected, got %d" % len(self.params))

    @staticmethod
    def parameter_names(sd_keys) -> List[str]:
        return sorted(k for k in sd_keys if k.startswith(PLANE_PREFIX) and k[len(PLANE_PREFIX):].split(".")[0] in PLANE_INSTANCE_HEADS)

    @classmethod
    def from_state_dict(cls, sd: dict, nq: int, device, cfg=None) -> "PlaneInstanceHeadsTrainer":
        return cls(cls._read(sd, cls.parameter_names(sd.keys()), device), nq, cfg)

    @classmethod
    def from_head(cls, head, cfg=None) -> "PlaneInstanceHeadsTrainer":
        return cls(cls._read(head, cls.parameter_names(cls._head_keys(head))), head.num_queries, cfg)

    # ---- forward
    def forward(self, hs: torch.Tensor, p1: torch.Tensor) -> dict:
        """hs [L, B, nq, 256] (hs[i] = the normed output of decoder layer 6 - L + i), p1 [B, h, w, 256] pixel-dense NHWC -> the reference's
        training dict: the last layer's pred_logits [B, nq, 2], pred_mask_logits [B, nq, h, w], pred_centers [B, nq, 2], pred_params
        [B, nq, 3] and pixel_centers [B, 2, h, w], and for L > 1 aux_outputs = the same four of the layers 0 .. L - 2 - the last layer
        first, the form PlaneCriterion takes.  Autograd tape attached."""
        P, nq = self.params, self.nq
        _require(hs.dim() == 4 and hs.shape[2] == nq and hs.shape[3] == 256 and 1 <= hs.shape[0] <= 3 and hs.dtype == torch.float32,
                 "PlaneInstanceHeadsTrainer: hs [L <= 3, B, %d, 256] f32 expected, got %s" % (nq, tuple(hs.shape)))
        L, B = hs.shape[:2]
        _require(p1.dim() == 4 and p1.shape[0] == B and p1.shape[3] == 256 and p1.dtype == torch.float32,
                 "PlaneInstanceHeadsTrainer: p1 [%d, h, w, 256] f32 expected, got %s" % (B, tuple(p1.shape)))
        q = PLANE_PREFIX
        x = hs.reshape(L * B * nq, 256)
        emb = _mlp_stack(P, q + "plane_embedding", x)                                 # (MLP: planeTR_head.py:194-206)
        w_pe = P[q + "pixel_embedding.weight"].view(256, 256)
        w_fold = torch.cat([w_pe.t(), P[q + "pixel_embedding.bias"].view(1, 256), w_pe.new_zeros(FOLD_WIDTH - 257, 256)], 0)
        fold = _linear(emb, w_fold)
        logits = _linear(x, P[q + "plane_prob.weight"], P[q + "plane_prob.bias"]).view(L, B, nq, -1)
        params = _mlp_stack(P, q + "plane_param", x).view(L, B, nq, 3)
        centers = _mlp_stack(P, q + "plane_center", x, ops.ACT_SIGMOID).view(L, B, nq, 2)
        masks, pixel_centers = _MaskProduct.apply(fold, p1, P[q + "pixel_plane_center.weight"], P[q + "pixel_plane_center.bias"], L, B, nq)
        layer = lambda l: {"pred_logits": logits[l], "pred_mask_logits": masks[l], "pred_centers": centers[l], "pred_params": params[l]}
        out = layer(L - 1)
        out["pixel_centers"] = pixel_centers
        if L > 1:
            out["aux_outputs"] = [layer(l) for l in range(L - 1)]
        return out

    def losses(self, hs: torch.Tensor, p1: torch.Tensor, targets: dict, num_masks=None, groups: int = 1):
        """-> (losses, indices) of PlaneCriterion.from_cfg on forward(hs, p1), the autograd tape attached; hs / p1 may require grad (their
        gradients land in `input_grads` after backward()).  groups: the criterion's view groups (2 for the two views of a 2B batch)."""
        out = self.forward(hs, p1)
        self._watch({"hs": hs, "p1": p1})
        self.last = out
        return self.criterion(out, targets, num_masks, groups)

    def backward(self, losses: Dict[str, torch.Tensor], loss_weights: Optional[Dict[str, float]] = None) -> Dict[str, torch.Tensor]:
        """d (sum of the losses under criterion.weighted's weights, or under `loss_weights`) / d parameters -> {state-dict key: gradient}."""
        if loss_weights is None:
            return super().backward(self.criterion.weighted(losses))
        return super().backward(losses, loss_weights)


class _LayerNormPair(torch.autograd.Function):
    """(y, y + addend) of one ops.layernorm launch, the addend [rows_a, 256] broadcast over the rows / rows_a sets (the decoder's query
    embedding).  Backward: ops.layernorm_backward on the sum of the two incoming gradients; the addend's gradient is the second one summed
    over the sets (ops.col_sum, fixed order)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, addend):
        x, addend = x.contiguous(), addend.contiguous()
        ctx.save_for_backward(x, gamma)
        ctx.a_shape = tuple(addend.shape)
        return ops.layernorm(x, gamma, beta, addend=addend, eps=LN_EPS)

    @staticmethod
    def backward(ctx, g_y, g_y2):
        x, gamma = ctx.saved_tensors
        dx, dgamma, dbeta = ops.layernorm_backward(x, gamma, (g_y + g_y2).contiguous(), LN_EPS)
        d_add = None
        if ctx.needs_input_grad[3]:
            n = ctx.a_shape[0] * ctx.a_shape[1]
            d_add = col_sum(g_y2.contiguous().view(-1, n)).view(ctx.a_shape)
        return dx, dgamma, dbeta, d_add


class _AddRows(torch.autograd.Function):
    """a + b with b [rows_b, D] broadcast over blocks of rows_b rows and constant (the sine position embedding on the encoder memory)."""

    @staticmethod
    def forward(ctx, a, b):
        return ops.add_rows(a.contiguous(), b.contiguous())

    @staticmethod
    def backward(ctx, g):
        return g, None


class _DecoderAttention(torch.autograd.Function):
    """Attention of the decoder (f32, head dim 32, any Lq / Lk).  Forward at p = 0: ops.attention, the inference head's own launch; at
    p > 0: ops.attention_train, dropout on the probabilities.  Backward: ops.attention_train_backward either way - it recomputes the
    softmax statistics and the mask, so it needs nothing from the forward launch."""

    @staticmethod
    def forward(ctx, q, k, v, B: int, Lq: int, Lk: int, heads: int, scale: float, p: float, seed: int, stream: int):
        if p == 0.0:
            o = ops.attention(q, k, v, B, Lq, Lk, heads, scale)
        else:
            o = ops.attention_train(q, k, v, B, Lq, Lk, heads, scale, p=p, seed=seed, stream=stream)
        ctx.conf = (B, Lq, Lk, heads, float(scale), float(p), int(seed), int(stream))
        ctx.save_for_backward(q, k, v)
        return o

    @staticmethod
    def backward(ctx, g):
        q, k, v = ctx.saved_tensors
        B, Lq, Lk, heads, scale, p, seed, stream = ctx.conf
        dq, dk, dv = ops.attention_train_backward(q, k, v, g.contiguous(), B, Lq, Lk, heads, scale, p=p, seed=seed, stream=stream)
        return dq, dk, dv, None, None, None, None, None, None, None, None


class _Dropout(torch.autograd.Function):
    """keep ? x / (1 - p) : 0 [+ residual] (ops.dropout, the mask from the counter); backward: the same kernel on the gradient."""

    @staticmethod
    def forward(ctx, x, residual, p: float, seed: int, stream: int):
        ctx.conf = (float(p), int(seed), int(stream))
        return ops.dropout(x.contiguous(), p, seed, stream, residual=None if residual is None else residual.contiguous())

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        gx = ops.dropout(g, *ctx.conf) if ctx.needs_input_grad[0] else None
        return gx, (g if ctx.needs_input_grad[1] else None), None, None, None


DECODER_LAYERS, DECODER_HEADS = 6, 8
DROP_SELF_ATTN, DROP_1, DROP_CROSS_ATTN, DROP_2, DROP_FFN, DROP_3 = range(6)         # the dropout sites of a layer (ops.dropout_stream)


class PlaneDecoderTrainer(ChainedTrainer):
    """The plane head's transformer decoder in TRAINING mode (reference: transformer/transformer.py:114-153, 293-322 as planeTR_head.py:88
    builds it - six pre-norm layers, dropout 0.1, return_intermediate): the 111 tensors of context2plane_decoder (per layer
    self_attn / multihead_attn in_proj + out_proj, linear1, linear2, norm1-3; the final norm) and query_embed.weight, held under their
    state-dict keys.  The encoder, the pyramid and the backbone stay frozen: the encoder's output enters as an input.

        memory, pos, p1 = model.sem_seg_head.decoder_training_inputs(features)     # [B*Lm, 256], [Lm, 256], [B, h, w, 256] (no autograd)
        dec = PlaneDecoderTrainer.from_head(model.sem_seg_head)                    # or .from_state_dict(sd, nq, device)
        hs = dec.forward(memory, pos, B, p=0.1, seed=seed, step=it)                # [L, B, nq, 256], autograd tape attached
        dec.backward_from(d_hs)                                                    # .grads, .input_grads["memory"]
      or, chained in front of the instance heads and the criterion:
        heads = PlaneInstanceHeadsTrainer.from_head(model.sem_seg_head)
        losses, indices = dec.losses(heads, memory, pos, p1, targets, p=0.1, seed=seed, step=it)
        dec.backward(losses); dec.step_from_cfg(cfg); heads.step_from_cfg(cfg)

    At p = 0 every launch of the forward is the launch PlaneTRHead._transformer_f32 makes on its f32 route, so the same parameters give
    PlaneTRHead.training_inputs' hs bit for bit.  At p > 0 the six dropout sites of every layer are active (attention probabilities
    inside ops.attention_train, the three residual branches and the FFN's hidden layer through ops.dropout); the masks are functions of
    (seed, step * 64 + layer * 8 + site, element index) and are recomputed by the backward kernels, never stored.  in_proj_weight / bias
    are one leaf each: their q | k rows and v rows enter the Linears as autograd views.  query_embed is the broadcast addend of norm1 and
    norm2; its gradient is summed over the batch.  Optimiser groups (train_NopeSAC.py:88-135): the LayerNorm tensors take
    WEIGHT_DECAY_NORM, query_embed (an nn.Embedding) WEIGHT_DECAY_EMBED, and the learning rate carries SOLVER.SEM_SEG_HEAD_MULTIPLIER."""

    KEY_PREFIX, LR_MULTIPLIER, OUTPUT = PLANE_PREFIX, "SEM_SEG_HEAD_MULTIPLIER", "hs"

    def __init__(self, params: Dict[str, torch.Tensor], nq: int, deep_supervision: bool = True):
        super().__init__(params)
        self.nq = int(nq)
        self.layers_out = 3 if deep_supervision else 1
        _require(len(self.params) == 18 * DECODER_LAYERS + 3, "PlaneDecoderTrainer: 111 tensors expected, got %d" % len(self.params))
        _require(self.params[PLANE_PREFIX + "query_embed.weight"].shape == (self.nq, 256), "PlaneDecoderTrainer: query_embed.weight [nq, 256]")

    @staticmethod
    def parameter_names(sd_keys) -> List[str]:
        return sorted(k for k in sd_keys if k.startswith(PLANE_PREFIX + DECODER + ".") or k == PLANE_PREFIX + "query_embed.weight")

    @classmethod
    def from_state_dict(cls, sd: dict, nq: int, device, deep_supervision: bool = True) -> "PlaneDecoderTrainer":
        return cls(cls._read(sd, cls.parameter_names(sd.keys()), device), nq, deep_supervision)

    @classmethod
    def from_head(cls, head) -> "PlaneDecoderTrainer":
        return cls(cls._read(head, cls.parameter_names(cls._head_keys(head))), head.num_queries, head.deep_supervision)

    # ---- forward
    def forward(self, memory: torch.Tensor, pos: torch.Tensor, B: int, p: float = 0.0, seed: int = 0, step: int = 0) -> torch.Tensor:
        """memory [B*Lm, 256] f32 (the encoder's output, rows in (b, token) order), pos [Lm, 256] -> hs [L, B, nq, 256]: the final norm of
        the outputs of the last L decoder layers (L = 3 under deep supervision, else 1), autograd tape attached.  p: the dropout rate
        (0 = the inference head's launches), seed / step: the counter's seed and the training step the masks are drawn for."""
        P, nq, nh = self.params, self.nq, DECODER_HEADS
        p = float(p)
        _require(memory.dim() == 2 and memory.shape[1] == 256 and memory.dtype == torch.float32 and B > 0 and memory.shape[0] % B == 0,
                 "PlaneDecoderTrainer: memory [B*Lm, 256] f32 expected, got %s" % (tuple(memory.shape),))
        Lm = memory.shape[0] // B
        _require(tuple(pos.shape) == (Lm, 256) and pos.dtype == torch.float32, "PlaneDecoderTrainer: pos [%d, 256] f32 expected, got %s" % (Lm, tuple(pos.shape)))
        mem = memory if memory.requires_grad else memory.detach().requires_grad_(True)
        self._watch({"memory": mem})                       # (its gradient: the value path and the key path, mem_k = memory + pos, summed)
        mem_k = _AddRows.apply(mem, pos.detach())
        scale = 32 ** -0.5
        qpos = P[PLANE_PREFIX + "query_embed.weight"]
        site = lambda i, s: ops.dropout_stream(step, i, s)
        att = lambda q, k, v, Lk, i, s: _DecoderAttention.apply(q, k, v, B, nq, Lk, nh, scale, p, int(seed), site(i, s))

        def out_proj(o, w, b, tgt, i, s):              # tgt + dropout(o W^T + b)
            if p == 0.0:
                return _linear(o, w, b, residual=tgt)
            return _Dropout.apply(_linear(o, w, b), tgt, p, int(seed), site(i, s))

        tgt = torch.zeros(B * nq, 256, device=memory.device, dtype=torch.float32)
        norm = (P[f"{PLANE_PREFIX}{DECODER}.norm.weight"], P[f"{PLANE_PREFIX}{DECODER}.norm.bias"])
        inter = []
        for i in range(DECODER_LAYERS):
            q = f"{PLANE_PREFIX}{DECODER}.layers.{i}."
            w, b = P[q + "self_attn.in_proj_weight"], P[q + "self_attn.in_proj_bias"]
            t2, q_in = _LayerNormPair.apply(tgt, P[q + "norm1.weight"], P[q + "norm1.bias"], qpos)
            qk = _linear(q_in, w[:512], b[:512])
            v = _linear(t2, w[512:], b[512:])
            o = att(qk[:, :256], qk[:, 256:], v, nq, i, DROP_SELF_ATTN)
            tgt = out_proj(o, P[q + "self_attn.out_proj.weight"], P[q + "self_attn.out_proj.bias"], tgt, i, DROP_1)
            w, b = P[q + "multihead_attn.in_proj_weight"], P[q + "multihead_attn.in_proj_bias"]
            t2, q_in = _LayerNormPair.apply(tgt, P[q + "norm2.weight"], P[q + "norm2.bias"], qpos)
            qc = _linear(q_in, w[:256], b[:256])
            kc = _linear(mem_k, w[256:512], b[256:512])
            vc = _linear(mem, w[512:], b[512:])
            o = att(qc, kc, vc, Lm, i, DROP_CROSS_ATTN)
            tgt = out_proj(o, P[q + "multihead_attn.out_proj.weight"], P[q + "multihead_attn.out_proj.bias"], tgt, i, DROP_2)
            t2 = _LayerNorm.apply(tgt, P[q + "norm3.weight"], P[q + "norm3.bias"], None)
            hdn = _linear(t2, P[q + "linear1.weight"], P[q + "linear1.bias"], ops.ACT_RELU)
            if p != 0.0:
                hdn = _Dropout.apply(hdn, None, p, int(seed), site(i, DROP_FFN))
            tgt = out_proj(hdn, P[q + "linear2.weight"], P[q + "linear2.bias"], tgt, i, DROP_3)
            if i >= DECODER_LAYERS - self.layers_out:
                inter.append(_LayerNorm.apply(tgt, norm[0], norm[1], None))
        self._out = torch.stack(inter).view(self.layers_out, B, nq, 256)
        return self._out

    def losses(self, heads: "PlaneInstanceHeadsTrainer", memory: torch.Tensor, pos: torch.Tensor, p1: torch.Tensor, targets: dict, p: float = 0.0,
               seed: int = 0, step: int = 0, num_masks=None, groups: int = 1):
        """Decoder, then the instance heads, then their PlaneCriterion: -> (losses, indices) of heads.losses on this forward's hs.  groups:
        the criterion's view groups; the decoder itself couples no two images."""
        self._heads = heads
        return heads.losses(self.forward(memory, pos, p1.shape[0], p, seed, step), p1, targets, num_masks, groups)


PYRAMID_CONVS = ("up_conv3", "up_conv2", "up_conv1", "c4_conv", "c3_conv", "c2_conv", "c1_conv", "m_conv_dict.m4")
PYRAMID_BN_EPS, PYRAMID_BN_MOMENTUM = 1e-5, 0.1                   # nn.BatchNorm2d's defaults (planeTR_head.py:212)


def _bn_statistics(src, up: bool, run_mean, run_var, batch_stats: bool, groups: int = 1):
    """(mean, rstd) of a pyramid BatchNorm: the batch's - per view group, [groups, C], for groups > 1 - with the running buffers updated
    in place (group after group), or the stored ones."""
    if batch_stats:
        mean, _var, rstd = ops.bn_train_stats(src, up=up, eps=PYRAMID_BN_EPS, momentum=PYRAMID_BN_MOMENTUM, running_mean=run_mean,
                                              running_var=run_var, groups=groups)
        return mean, rstd
    return run_mean, torch.rsqrt(run_var + PYRAMID_BN_EPS)


class _ConvBNTrain(torch.autograd.Function):
    """A block of the top-down pyramid with a training-mode BatchNorm (batch statistics, the running buffers updated in place) or,
    batch_stats=False, with the stored statistics as constants.  up=False, a lateral: relu(bn(conv1x1(x))) (+ addend).  up=True, an up
    stage: relu(bn(conv1x1(up2(x)))) + addend, evaluated as relu(bn(up2(c))) + addend with c = conv1x1(x) at the LOW resolution (the 1x1
    conv commutes with the bilinear interpolation, PlaneTRHead._pyramid); the batch statistics are those of up2(c), which the kernels
    evaluate on the fly, and the backward gathers the bilinear adjoint inside the BatchNorm backward's launch.  The raw conv output is
    saved; the conv's dgrad / wgrad run at its own (low) resolution.  groups > 1 (with batch statistics): the images are that many view
    groups, each normalised by its own statistics; the conv and its gradients are per pixel and take the whole batch."""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, addend, run_mean, run_var, batch_stats: bool, up: bool, groups: int = 1):
        x = x.contiguous()
        c = ops.conv2d(x, _ohwi(w, x.shape[3]))
        G = int(groups) if batch_stats else 1
        mean, rstd = _bn_statistics(c, up, run_mean, run_var, batch_stats, G)
        ctx.conf = (batch_stats, up, G)
        ctx.save_for_backward(x, w, c, gamma, beta, mean, rstd)
        return ops.bn_train_apply(c, gamma, beta, mean, rstd, ops.ACT_RELU, None if addend is None else addend.contiguous(), up=up, groups=G)

    @staticmethod
    def backward(ctx, g):
        x, w, c, gamma, beta, mean, rstd = ctx.saved_tensors
        batch_stats, up, G = ctx.conf
        g = g.contiguous()
        dc, dgamma, dbeta = ops.bn_train_backward(g, c, gamma, beta, mean, rstd, ops.ACT_RELU, up=up, batch_stats=batch_stats, groups=G)
        dx, dw = _conv_input_grads(ctx, x, w, dc, 1, 0)
        return dx, dw, dgamma, dbeta, (g if ctx.needs_input_grad[4] else None), None, None, None, None, None


class PlanePyramidTrainer(ChainedTrainer):
    """The plane head's top-down pyramid in TRAINING mode (reference top_down, planeTR_head.py:209-252, unfrozen: cfg.MODEL.FREEZE = []):
    eight 1x1 convs without bias, each followed by an nn.BatchNorm2d on BATCH statistics and a ReLU - 24 parameters (conv weight, BN
    weight, BN bias) under their state-dict keys, plus the 16 running-statistics buffers and the eight num_batches_tracked counters
    (`buffers`), which a batch-statistics forward updates on the device as torch does (momentum 0.1, unbiased variance).

        memory, feats = model.sem_seg_head.pyramid_training_inputs(features)       # [B*Lm, 256], {res2 .. res5: f32 NHWC} (no autograd)
        pyr = PlanePyramidTrainer.from_head(model.sem_seg_head)                    # or .from_state_dict(sd, device)
        p1 = pyr.forward(feats, memory, B)                                         # [B, h, w, 256], autograd tape attached
        pyr.backward_from(d_p1)                                                    # .grads, .input_grads["memory"] (and "res2" .. "res5")
      or, chained in front of the instance heads and the criterion:
        losses, indices = pyr.losses(heads, feats, memory, hs, targets)
        pyr.backward(losses); pyr.step_from_cfg(cfg); heads.step_from_cfg(cfg); pyr.write_back(model.sem_seg_head)

    `memory` may be a leaf that requires grad and that PlaneDecoderTrainer.forward consumes too: then autograd sums both paths into the
    total gradient at the encoder's output.  batch_stats=False runs on the stored statistics (the reference's FrozenBatchNorm2d regime:
    the same kernels with mean / rstd as constants of the backward) and leaves the buffers untouched.  Up stages keep the inference
    head's algebra (the conv at the low resolution).  Optimiser groups (train_NopeSAC.py:88-135): the 16 BatchNorm affine tensors take
    WEIGHT_DECAY_NORM; the learning rate carries SOLVER.SEM_SEG_HEAD_MULTIPLIER."""

    KEY_PREFIX, LR_MULTIPLIER, OUTPUT = PLANE_PREFIX, "SEM_SEG_HEAD_MULTIPLIER", "p1"

    def __init__(self, params: Dict[str, torch.Tensor], buffers: Dict[str, torch.Tensor], feature_grads: bool = False):
        super().__init__(params)
        self.feature_grads = bool(feature_grads)
        self.buffers = {k: (v.detach().clone().to(torch.int64) if k.endswith("num_batches_tracked") else v.detach().clone().float().contiguous())
                        for k, v in buffers.items()}
        _require(len(self.params) == 24 and len(self.buffers) == 24,
                 "PlanePyramidTrainer: 24 parameters and 24 buffers expected, got %d and %d" % (len(self.params), len(self.buffers)))

    @staticmethod
    def _names(sd_keys, buffers: bool) -> List[str]:
        q = PLANE_PREFIX + TOP_DOWN + "."
        return sorted(k for k in sd_keys if k.startswith(q) and (k.split(".")[-1] in _BUFFER_LEAVES) == buffers)

    @staticmethod
    def parameter_names(sd_keys) -> List[str]:
        return PlanePyramidTrainer._names(sd_keys, False)

    @staticmethod
    def buffer_names(sd_keys) -> List[str]:
        return PlanePyramidTrainer._names(sd_keys, True)

    @classmethod
    def from_state_dict(cls, sd: dict, device, feature_grads: bool = False) -> "PlanePyramidTrainer":
        keys = list(sd.keys())
        return cls(cls._read(sd, cls.parameter_names(keys), device), cls._read(sd, cls.buffer_names(keys), device), feature_grads)

    @classmethod
    def from_head(cls, head, feature_grads: bool = False) -> "PlanePyramidTrainer":
        keys = cls._head_keys(head)
        return cls(cls._read(head, cls.parameter_names(keys)), cls._read(head, cls.buffer_names(keys)), feature_grads)

    def write_back(self, head):
        """Copy the trained tensors AND the running statistics / counters into the inference PlaneTRHead and drop its packed copies (the
        BatchNorm folds among them: rebuilt on the next forward)."""
        self._copy_into(head, {**self.params, **self.buffers})

    # ---- forward
    def forward(self, feats: dict, memory: torch.Tensor, B: int, batch_stats: bool = True, groups: int = 1) -> torch.Tensor:
        """feats: res2 .. res5 f32 NHWC ([B, h, w, 256 / 512 / 1024 / 2048], each level twice the next one's size), memory [B*Lm, 256] f32 with
        Lm = res5's pixels -> p1 [B, h2, w2, 256], the pixel decoder's map at res2's resolution, autograd tape attached.
        groups = G: the B images are G view groups of B / G consecutive ones (groups=2: both views of a pair batch, view 1 first), and every
        BatchNorm takes its batch statistics per group, updates its running buffers group after group and counts G batches - what the
        reference's G top_down calls leave; p1 of a group has the bits of a forward on that group alone.  batch_stats=False ignores it."""
        P, Bf = self.params, self.buffers
        G = int(groups) if batch_stats else 1
        _require(G >= 1 and B % G == 0, "PlanePyramidTrainer: groups=%d does not divide the batch of %d" % (G, B))
        c = {}
        for k in ("res2", "res3", "res4", "res5"):
            t = feats[k]
            _require(t.dim() == 4 and t.shape[0] == B and t.dtype == torch.float32, "PlanePyramidTrainer: %s [%d, h, w, C] f32 expected, got %s" % (k, B, tuple(t.shape)))
            c[k] = t.detach().requires_grad_(True) if self.feature_grads and not t.requires_grad else t
        hc, wc = c["res5"].shape[1:3]
        for k, f in (("res4", 2), ("res3", 4), ("res2", 8)):
            _require(tuple(c[k].shape[1:3]) == (f * hc, f * wc), "PlanePyramidTrainer: %s must be %d x res5's size" % (k, f))
        _require(tuple(memory.shape) == (B * hc * wc, 256) and memory.dtype == torch.float32,
                 "PlanePyramidTrainer: memory [%d, 256] f32 expected, got %s" % (B * hc * wc, tuple(memory.shape)))
        mem = memory if memory.requires_grad else memory.detach().requires_grad_(True)
        self._watch(dict({"memory": mem}, **{k: t for k, t in c.items() if t.requires_grad}))       # (memory: through m_conv_dict.m4)
        bs = bool(batch_stats)

        def stage(up, x, nm, other):
            q = f"{PLANE_PREFIX}{TOP_DOWN}.{nm}"
            y = _ConvBNTrain.apply(x, P[q + ".0.weight"], P[q + ".1.weight"], P[q + ".1.bias"], other, Bf[q + ".1.running_mean"],
                                   Bf[q + ".1.running_var"], bs, up, G)
            if bs:
                Bf[q + ".1.num_batches_tracked"] += G
            return y
        p4 = stage(False, mem.view(B, hc, wc, 256), "m_conv_dict.m4", stage(False, c["res5"], "c4_conv", None))
        p3 = stage(True, p4, "up_conv3", stage(False, c["res4"], "c3_conv", None))
        p2 = stage(True, p3, "up_conv2", stage(False, c["res3"], "c2_conv", None))
        self._out = stage(True, p2, "up_conv1", stage(False, c["res2"], "c1_conv", None))
        return self._out

    def losses(self, heads: "PlaneInstanceHeadsTrainer", feats: dict, memory: torch.Tensor, hs: torch.Tensor, targets: dict,
               batch_stats: bool = True, num_masks=None, groups: int = 1):
        """Pyramid, then the instance heads, then their PlaneCriterion: -> (losses, indices) of heads.losses on this forward's p1 (under deep
        supervision p1 feeds every supervised layer's masks).  hs [L, B, nq, 256]: constants, or PlaneDecoderTrainer.forward's output.
        groups: the view groups of the BatchNorm statistics and of the criterion alike."""
        self._heads = heads
        return heads.losses(hs, self.forward(feats, memory, hs.shape[1], batch_stats, groups), targets, num_masks, groups)


class _ConvBiasInPlace(torch.autograd.Function):
    """_ConvBias for a 1x1 conv (input_proj): the same forward launch; backward: one ops.linear_backward call on the pixels as rows."""

    @staticmethod
    def forward(ctx, x, w, b):
        x = x.contiguous()
        ctx.save_for_backward(x, w)
        return ops.conv2d(x, _ohwi(w, x.shape[3]), bias=b.detach().contiguous())

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        Cout, Cin = w.shape[:2]
        dx, dw, db = ops.linear_backward(x.view(-1, Cin), w.view(Cout, Cin), g.contiguous().view(-1, Cout), want=tuple(ctx.needs_input_grad))
        return (None if dx is None else dx.view(x.shape)), (None if dw is None else dw.view(w.shape)), db


class _EncoderAttention(torch.autograd.Function):
    """Self attention of an encoder layer on qk = q | k [rows, 512] (one N = 512 Linear on src + pos) and v [rows, 256].  Forward at
    p = 0: ops.attention, the inference head's launch; at p > 0: ops.attention_train.  Backward: ops.attention_train_backward, which
    writes dq and dk straight into the two halves of one [rows, 512] gradient."""

    @staticmethod
    def forward(ctx, qk, v, B: int, L: int, heads: int, scale: float, p: float, seed: int, stream: int):
        W = heads * 32
        qk, v = qk.contiguous(), v.contiguous()
        if p == 0.0:
            o = ops.attention(qk[:, :W], qk[:, W:], v, B, L, L, heads, scale)
        else:
            o = ops.attention_train(qk[:, :W], qk[:, W:], v, B, L, L, heads, scale, p=p, seed=seed, stream=stream)
        ctx.conf = (B, L, heads, float(scale), float(p), int(seed), int(stream))
        ctx.save_for_backward(qk, v)
        return o

    @staticmethod
    def backward(ctx, g):
        qk, v = ctx.saved_tensors
        B, L, heads, scale, p, seed, stream = ctx.conf
        W = heads * 32
        dqk, dv = torch.empty_like(qk), torch.empty_like(v)
        ops.attention_train_backward(qk[:, :W], qk[:, W:], v, g.contiguous(), B, L, L, heads, scale, p=p, seed=seed, stream=stream,
                                     out=(dqk[:, :W], dqk[:, W:], dv))
        return dqk, dv, None, None, None, None, None, None, None


ENCODER_LAYERS, ENCODER_HEADS = 6, 8
ENC_DROP_ATTN, ENC_DROP_1, ENC_DROP_FFN, ENC_DROP_2 = range(4)                       # the dropout sites of a layer (ops.encoder_dropout_stream)


class PlaneEncoderTrainer(ChainedTrainer):
    """The plane head's transformer encoder in TRAINING mode (reference: planeTR_head.py:77-82, 125-132 and transformer/transformer.py:
    183-199 with normalize_before=False, dropout 0.1): input_proj (the 1x1 conv 2048 -> 256 on res5), the six post-norm layers of
    context_SA (self_attn in_proj + out_proj, linear1, linear2, norm1, norm2) and the final norm - 76 tensors under their state-dict
    keys.  With it all 235 tensors of sem_seg_head train through one graph; only the backbone stays behind.

        feats, pos = model.sem_seg_head.encoder_training_inputs(features)          # {res2 .. res5: f32 NHWC}, [Lm, 256] (no autograd)
        enc = PlaneEncoderTrainer.from_head(model.sem_seg_head)                    # or .from_state_dict(sd, device)
        memory = enc.forward(feats["res5"], B, p=0.1, seed=seed, step=it)          # [B*Lm, 256], autograd tape attached
        enc.backward_from(d_memory)                                                # d_memory: the decoder's + the pyramid's input_grads["memory"]
      or the whole head on one graph:
        losses, indices = enc.losses(heads, decoder, pyramid, feats, targets, p=0.1, seed=seed, step=it)
        grads = enc.backward(losses)                                               # all 235 tensors by key; each trainer's .grads is filled

    At p = 0 every launch of the forward is the launch PlaneTRHead._encoder_f32 makes on its f32 route (input_proj included), so the same
    parameters give decoder_training_inputs' memory bit for bit.  At p > 0 the four dropout sites of every layer are active: the
    attention probabilities inside ops.attention_train, the two residual branches as ops.dropout(branch, residual=src) behind a plain
    Linear, the FFN's hidden layer through ops.dropout behind its ReLU; the masks are functions of
    (seed, ops.encoder_dropout_stream(step, layer, site), element index), recomputed in the backward, never stored.  in_proj_weight /
    bias are one leaf each: the q | k rows and the v rows enter the Linears as autograd views.  Every Linear goes through LINEAR:
    _LinearInPlace, whose backward is one ops.linear_backward call with the ReLU and dropout gates applied as the gradient is loaded
    (set LINEAR = _Linear for the composition of the other trainers: the same forward bits).  Optimiser groups (train_NopeSAC.py:88-135):
    the 26 LayerNorm tensors take WEIGHT_DECAY_NORM; the learning rate carries SOLVER.SEM_SEG_HEAD_MULTIPLIER."""

    KEY_PREFIX, LR_MULTIPLIER, OUTPUT = PLANE_PREFIX, "SEM_SEG_HEAD_MULTIPLIER", "memory"
    LINEAR = _LinearInPlace

    def __init__(self, params: Dict[str, torch.Tensor], feature_grads: bool = False, pos=None):
        super().__init__(params)
        self.feature_grads = bool(feature_grads)
        self._pos_of = pos                              # (h, w, device) -> the sine embedding [h w, 256]; default: the head's own function
        self._pos_cache: Dict[tuple, torch.Tensor] = {}
        self._chain = None
        _require(len(self.params) == 12 * ENCODER_LAYERS + 4, "PlaneEncoderTrainer: 76 tensors expected, got %d" % len(self.params))
        _require(self.LINEAR in (_LinearInPlace, _Linear), "PlaneEncoderTrainer.LINEAR: _LinearInPlace or _Linear (forward and _linear_site know these two)")

    @staticmethod
    def parameter_names(sd_keys) -> List[str]:
        return sorted(k for k in sd_keys if k.startswith(PLANE_PREFIX + ENCODER + ".") or k.startswith(PLANE_PREFIX + INPUT_PROJ + "."))

    @classmethod
    def from_state_dict(cls, sd: dict, device, feature_grads: bool = False) -> "PlaneEncoderTrainer":
        return cls(cls._read(sd, cls.parameter_names(sd.keys()), device), feature_grads)

    @classmethod
    def from_head(cls, head, feature_grads: bool = False) -> "PlaneEncoderTrainer":
        return cls(cls._read(head, cls.parameter_names(cls._head_keys(head))), feature_grads, head._pos)

    def pos(self, h: int, w: int, device) -> torch.Tensor:
        """The head's sine position embedding of an h x w map, [h w, 256] f32 on `device`: a constant."""
        if self._pos_of is not None:
            return self._pos_of(h, w, device)
        key = (h, w, str(device))
        if key not in self._pos_cache:
            from .modeling.plane_head import sine_position_embedding
            self._pos_cache[key] = sine_position_embedding(h, w).to(device)
        return self._pos_cache[key]

    # ---- forward
    def _linear_site(self, x, w, b, act: int = ops.ACT_NONE, residual=None, p: float = 0.0, seed: int = 0, stream: int = 0):
        """act(x W^T + b), then (p > 0) the dropout that sits behind it, then + residual."""
        if self.LINEAR is _LinearInPlace:
            return _LinearInPlace.apply(x, w, b, act, residual, p, seed, stream)
        if p == 0.0:
            return self.LINEAR.apply(x, w, b, act, residual)
        return _Dropout.apply(self.LINEAR.apply(x, w, b, act, None), residual, p, seed, stream)

    def forward(self, res5: torch.Tensor, B: int, p: float = 0.0, seed: int = 0, step: int = 0, pos: Optional[torch.Tensor] = None) -> torch.Tensor:
        """res5 [B, h, w, 2048] f32 NHWC (pyramid_training_inputs' / encoder_training_inputs' feats["res5"]) -> memory [B*h*w, 256], the
        encoder's output with rows in (b, token) order, autograd tape attached.  p: the dropout rate (0 = the inference head's launches),
        seed / step: the counter's seed and the training step the masks are drawn for; pos [h w, 256]: the position embedding, if not the
        head's."""
        P, nh = self.params, ENCODER_HEADS
        p, seed = float(p), int(seed)
        _require(res5.dim() == 4 and res5.shape[0] == B and res5.shape[3] == 2048 and res5.dtype == torch.float32,
                 "PlaneEncoderTrainer: res5 [%d, h, w, 2048] f32 expected, got %s" % (B, tuple(res5.shape)))
        h, w = res5.shape[1:3]
        L = h * w
        pos = (self.pos(h, w, res5.device) if pos is None else pos).detach()
        _require(tuple(pos.shape) == (L, 256) and pos.dtype == torch.float32, "PlaneEncoderTrainer: pos [%d, 256] f32 expected, got %s" % (L, tuple(pos.shape)))
        c4 = res5.detach().requires_grad_(True) if self.feature_grads and not res5.requires_grad else res5
        self._watch({"res5": c4} if c4.requires_grad else {})
        q = PLANE_PREFIX + INPUT_PROJ
        if self.LINEAR is _LinearInPlace:
            src = _ConvBiasInPlace.apply(c4, P[q + ".weight"], P[q + ".bias"]).view(B * L, 256)
        else:
            src = _ConvBias.apply(c4, P[q + ".weight"], P[q + ".bias"], 0).view(B * L, 256)
        q_in = _AddRows.apply(src, pos)
        scale = 32 ** -0.5
        site = lambda i, s: ops.encoder_dropout_stream(step, i, s)
        for i in range(ENCODER_LAYERS):
            q = f"{PLANE_PREFIX}{ENCODER}.layers.{i}."
            wi, bi = P[q + "self_attn.in_proj_weight"], P[q + "self_attn.in_proj_bias"]
            qk = self._linear_site(q_in, wi[:512], bi[:512])
            v = self._linear_site(src, wi[512:], bi[512:])
            o = _EncoderAttention.apply(qk, v, B, L, nh, scale, p, seed, site(i, ENC_DROP_ATTN))
            s = self._linear_site(o, P[q + "self_attn.out_proj.weight"], P[q + "self_attn.out_proj.bias"], residual=src, p=p, seed=seed,
                          stream=site(i, ENC_DROP_1))
            src = _LayerNorm.apply(s, P[q + "norm1.weight"], P[q + "norm1.bias"], None)
            hdn = self._linear_site(src, P[q + "linear1.weight"], P[q + "linear1.bias"], ops.ACT_RELU, p=p, seed=seed, stream=site(i, ENC_DROP_FFN))
            s = self._linear_site(hdn, P[q + "linear2.weight"], P[q + "linear2.bias"], residual=src, p=p, seed=seed, stream=site(i, ENC_DROP_2))
            src, q_in = _LayerNormPair.apply(s, P[q + "norm2.weight"], P[q + "norm2.bias"], pos)
        q = f"{PLANE_PREFIX}{ENCODER}.norm."
        self._out, _ = _LayerNormPair.apply(src, P[q + "weight"], P[q + "bias"], pos)
        return self._out

    # ---- the whole head on one graph
    def losses(self, heads: "PlaneInstanceHeadsTrainer", decoder: "PlaneDecoderTrainer", pyramid: "PlanePyramidTrainer", feats: dict,
               targets: dict, p: float = 0.0, seed: int = 0, step: int = 0, batch_stats: bool = True, num_masks=None, groups: int = 1):
        """Encoder, then the decoder and the pyramid on this forward's memory, then the instance heads and their PlaneCriterion:
        -> (losses, indices) of heads.losses.  feats: res2 .. res5 f32 NHWC.  The decoder and the pyramid each take their own view of
        the one non-leaf memory, so each reports its own path in input_grads["memory"] and the encoder receives their two-term sum.
        groups: the view groups of the pyramid's BatchNorm statistics and of the criterion (2 for a 2B-image pair batch); the encoder
        and the decoder couple no two images."""
        res5 = feats["res5"]
        B, h, w = res5.shape[:3]
        memory = self.forward(res5, B, p, seed, step)
        if "res5" in self._inputs:                                  # the leaf the encoder watches is the pyramid's too: both paths sum
            feats = dict(feats, res5=self._inputs["res5"])
        hs = decoder.forward(memory.view_as(memory), self.pos(h, w, res5.device), B, p, seed, step)
        p1 = pyramid.forward(feats, memory.view_as(memory), B, batch_stats, groups)
        self._heads, self._chain = heads, (decoder, pyramid)
        return heads.losses(hs, p1, targets, num_masks, groups)

    def backward(self, losses: Dict[str, torch.Tensor], loss_weights: Optional[Dict[str, float]] = None) -> Dict[str, torch.Tensor]:
        """The chain's backward: the instance heads' backward runs on through the decoder and the pyramid into the encoder.  -> the
        gradients of all 235 tensors of sem_seg_head by state-dict key; every trainer's `.grads` / `.input_grads` is filled."""
        _require(self._heads is not None and self._chain is not None, "PlaneEncoderTrainer.backward: call losses() first (backward_from takes a gradient at memory)")
        chain = (self,) + tuple(self._chain)
        for t in chain:
            t._clear_grads()
        head_grads = self._heads.backward(losses, loss_weights)
        out: Dict[str, torch.Tensor] = {}
        for t in chain:
            out.update(t._collect())
        out.update(head_grads)
        return out


BACKBONE_PREFIX, FROZEN_BN_EPS = "backbone.", 1e-5
BACKBONE_MAPS = ("res2", "res3", "res4", "res5")


class _ConvFrozenBN(torch.autograd.Function):
    """conv (no bias) + FrozenBN (scale / shift constants) [+ residual] + act, as ONE ops.conv2d launch - the launch HipResNet50.forward
    makes on its f32 route.  Only x, w and the post-activation output are kept: the backward takes the ReLU gate from y > 0
    (ops.frozen_bn_act_backward), then dgrad (stride 1: ops.conv2d_dgrad, stride 2: ops.conv2d_dgrad_strided) and wgrad; the residual
    receives dz.  x may carry zero padding channels beyond w's Cin (the stem's fourth): their weight gradient is dropped."""

    @staticmethod
    def forward(ctx, x, w, scale, shift, residual, stride: int, pad: int, act: int):
        x = x.contiguous()
        y = ops.conv2d(x, _ohwi(w, x.shape[3]), scale, shift, residual, stride=stride, pad=pad, act=act)
        ctx.conf = (stride, pad, act)
        ctx.save_for_backward(x, w, y, scale)
        return y

    @staticmethod
    def backward(ctx, g):
        x, w, y, scale = ctx.saved_tensors
        stride, pad, act = ctx.conf
        want_dz = bool(ctx.needs_input_grad[4])
        r = ops.frozen_bn_act_backward(g.contiguous(), y, scale, act, want_dz)
        dc, dz = r if want_dz else (r, None)
        dx = dw = None
        B, H, W, Cx = x.shape
        Cin, k = w.shape[1], w.shape[2]
        if ctx.needs_input_grad[0]:
            _require(Cx == Cin, "_ConvFrozenBN: an input with padding channels takes no gradient")
            dx = torch.empty_like(x)
            if stride == 1:
                ops.conv2d_dgrad(dc, w, (H, W), stride=1, pad=pad, out=dx)
            else:
                ops.conv2d_dgrad_strided(dc, w, (H, W), stride=stride, pad=pad, out=dx)
        if ctx.needs_input_grad[1]:
            # (the wgrad kernel needs Cin % 4 == 0: the stem runs on all four channels of its padded input and drops the fourth)
            dw = ops.conv2d_wgrad(x, dc, k, stride=stride, pad=pad, cin=None)[:, :Cin] if Cx > Cin else \
                ops.conv2d_wgrad(x, dc, k, stride=stride, pad=pad, cin=Cin)
        return dx, dw, None, None, dz, None, None, None


class _MaxPool3(torch.autograd.Function):
    """The stem's 3x3 / stride-2 / pad-1 max-pool."""

    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        ctx.save_for_backward(x)
        return ops.maxpool(x, 3, 2, 1)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return ops.maxpool3x3s2_backward(x, g.contiguous())


class BackboneTrainer(HeadTrainer):
    """The ResNet-50 backbone in TRAINING mode as the reference trains it (configs/Base.yaml: FREEZE_AT 0, NORM FrozenBN,
    SOLVER.BACKBONE_MULTIPLIER 0.1): the trainable set is the 53 conv weights - the stem, 16 x 3 bottleneck convs, 4 projection
    shortcuts - under their state-dict keys; the FrozenBN scale / shift vectors (eps 1e-5) are constants folded once (`norms`).

        bb = BackboneTrainer.from_backbone(model.backbone)                         # or .from_state_dict(sd, device)
        feats = bb.forward(x)                                                      # x [N, H, W, 4] f32 normalised NHWC -> {res2 .. res5}
        bb.backward_from({"res5": d_res5, ...})                                    # any subset of the maps -> .grads (53 tensors)
      or with another trainer's graph behind the maps (they take tensors that require grad as they are):
        losses, _ = enc.losses(heads, decoder, pyramid, feats, targets)
        grads = bb.joined_backward(enc, losses)                                    # the 53 + the other trainer's, by state-dict key
        bb.step_from_cfg(cfg); bb.write_back(model.backbone)

    Every launch of the forward is the one HipResNet50.forward makes on its f32 route (one ops.conv2d per conv with scale, shift, residual
    and ReLU in the epilogue, ops.maxpool), so the same parameters give the inference backbone's f32 maps bit for bit.  Each returned map
    is a view of the activation the next stage consumes: its gradient is what the consumers behind the backbone send, not the
    backbone's own paths, so a consumer's `input_grads` is exactly what backward_from takes.  The backward is csrc/backbone_bwd.hip (the
    ReLU gate from the saved output, the stride-2 dgrad on the MFMA, the overlapping max-pool) plus conv2d_dgrad / conv2d_wgrad of
    csrc/conv_bwd.hip.  The image takes no gradient (the stem has no dgrad).  Optimiser group: all 53 are "plain"."""

    KEY_PREFIX, LR_MULTIPLIER = BACKBONE_PREFIX, "BACKBONE_MULTIPLIER"
    BLOCKS = {"res2": 3, "res3": 4, "res4": 6, "res5": 3}               # bottlenecks per stage (synth.RES_STAGES)

    def __init__(self, params: Dict[str, torch.Tensor], norms: Dict[str, tuple]):
        super().__init__(params)
        self.norms = {k: (s.detach().float().contiguous(), b.detach().float().contiguous()) for k, (s, b) in norms.items()}
        self._out: Dict[str, torch.Tensor] = {}
        _require(len(self.params) == 53 and set(self.norms) == {k[:-len(".weight")] for k in self.params},
                 "BackboneTrainer: 53 conv weights, each with its FrozenBN, expected, got %d and %d" % (len(self.params), len(self.norms)))

    @staticmethod
    def parameter_names(sd_keys) -> List[str]:
        return sorted(k for k in sd_keys if k.startswith(BACKBONE_PREFIX) and k.endswith(".weight") and ".norm." not in k)

    @classmethod
    def _build(cls, source, keys, device=None) -> "BackboneTrainer":
        names = cls.parameter_names(keys)
        norms = {}
        for k in names:
            q = k[:-len(".weight")]
            n = cls._read(source, [q + ".norm." + leaf for leaf in ("weight", "bias", "running_mean", "running_var")], device)
            w, b, mean, var = (t.float() for t in n.values())
            scale = w * torch.rsqrt(var + FROZEN_BN_EPS)                  # (modeling.params.fold_bn's expression: the same bits)
            norms[q] = (scale, b - mean * scale)
        return cls(cls._read(source, names, device), norms)

    @classmethod
    def from_state_dict(cls, sd: dict, device) -> "BackboneTrainer":
        return cls._build(sd, list(sd.keys()), device)

    @classmethod
    def from_backbone(cls, backbone) -> "BackboneTrainer":
        return cls._build(backbone, cls._head_keys(backbone))

    # ---- forward
    def _conv(self, x, name: str, stride: int = 1, pad: int = 0, act: int = ops.ACT_RELU, residual=None):
        scale, shift = self.norms[BACKBONE_PREFIX + name]
        return _ConvFrozenBN.apply(x, self.params[BACKBONE_PREFIX + name + ".weight"], scale, shift, residual, stride, pad, act)

    def forward(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        """x [N, H, W, 4] f32 NHWC, normalised, the fourth channel zero (ops.preprocess) -> {res2 .. res5} f32 NHWC, autograd tape attached."""
        x = self.stem(x)
        out = {}
        for name in BACKBONE_MAPS:
            x = self.stage(x, name)
            out[name] = x.view_as(x)
        self._out = out
        return out

    def stem(self, x: torch.Tensor) -> torch.Tensor:
        """The 7x7 / stride-2 conv on the 4-channel padded image and the 3x3 / stride-2 max-pool -> [N, H / 4, W / 4, 64]."""
        _require(x.dim() == 4 and x.shape[3] == 4 and x.dtype == torch.float32, "BackboneTrainer: x [N, H, W, 4] f32 expected, got %s" % (tuple(x.shape),))
        return _MaxPool3.apply(self._conv(x.detach(), "stem.conv1", 2, 3))

    def stage(self, x: torch.Tensor, name: str) -> torch.Tensor:
        """One of res2 .. res5 on the previous stage's output: its bottlenecks, the first with a projection shortcut (stride 2 in its
        3x3 conv and its shortcut, except res2)."""
        for i in range(self.BLOCKS[name]):
            p = f"{name}.{i}"
            stride = 2 if (i == 0 and name != "res2") else 1
            y = self._conv(x, p + ".conv1")
            y = self._conv(y, p + ".conv2", stride, 1)
            sc = self._conv(x, p + ".shortcut", stride, 0, ops.ACT_NONE) if i == 0 else x
            x = self._conv(y, p + ".conv3", residual=sc)
        return x

    # ---- backward
    def backward_from(self, d_feats: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """Gradients at any subset of the last forward's maps ({"res2" .. "res5": like the map}) -> {state-dict key: gradient} of the 53
        weights (also `.grads`)."""
        _require(self._out and d_feats and all(k in self._out and tuple(g.shape) == tuple(self._out[k].shape) for k, g in d_feats.items()),
                 "BackboneTrainer.backward_from: {res2 .. res5: gradient like the last forward's map}")
        keys = [k for k in BACKBONE_MAPS if k in d_feats]
        self._clear_grads()
        torch.autograd.backward([self._out[k] for k in keys], [d_feats[k].contiguous() for k in keys])
        return self._collect()

    def joined_backward(self, trainer: HeadTrainer, losses: Dict[str, torch.Tensor], loss_weights: Optional[Dict[str, float]] = None) -> Dict[str, torch.Tensor]:
        """The backward of a graph that runs on from this forward's maps into another trainer (its losses / forward were given the maps
        themselves): `trainer.backward(losses, loss_weights)` continues into the backbone.  -> both trainers' gradients by state-dict
        key; `.grads` here holds the backbone's 53."""
        _require(bool(self._out), "BackboneTrainer.joined_backward: call forward() first")
        self._clear_grads()
        other = trainer.backward(losses, loss_weights)
        return {**self._collect(), **other}


def plane_corr_matrix(gt_corrs: torch.Tensor, match1: torch.Tensor, match2: torch.Tensor, nq: int) -> torch.Tensor:
    """gt correspondences of the predicted planes (process_plane_corr_matrix, siamese_planeTR.py:566-623) in the form
    MatchingHeadTrainer.matching_losses takes: gt_corrs int32 [B, K, 2] on the device (rows padded with -1), match1 / match2 = the two
    views' indices["match_q"][0] -> uint8 [B, nq+1, nq+1].  One launch, no host sync."""
    return ops.plane_corr_matrix(gt_corrs.contiguous(), match1.contiguous(), match2.contiguous(), nq)


# ---- the two-view half of the training forward (siamese_planeTR.py:237-299) ----------------------------------------------------------------
class _MatchCompact(torch.autograd.Function):
    """ops.match_compact with the queries on the tape: (x_c, params_c, order, rank, bad); the backward is the scatter back through `rank`.
    params_c carries no gradient (the matcher detaches its geometry, matching_head.py:98-99)."""

    @staticmethod
    def forward(ctx, x, params, match_q, n):
        x_c, params_c, order, rank, bad = ops.match_compact(x.contiguous(), params.detach().contiguous(), match_q.contiguous(), n.contiguous())
        ctx.save_for_backward(rank)
        ctx.mark_non_differentiable(params_c, order, rank, bad)
        return x_c, params_c, order, rank, bad

    @staticmethod
    def backward(ctx, g_x_c, _p, _o, _r, _b):
        (rank,) = ctx.saved_tensors
        return ops.match_compact_backward(g_x_c.contiguous(), rank), None, None, None


_RAND_POSE_SALT = 0x52414E44504F5345       # keeps the draws apart from augment.sample_params' for the same (seed, step, row)


def sample_rand_poses(count: int, seed: int = 0, step: int = 0):
    """The AIM's random poses (camera_head.py:688-691, :716): a rotation vector uniform in (-2.5, 2.5)^3 turned into a unit quaternion
    (w, x, y, z), a translation uniform in (-2.5, 2.5)^3 -> (rot f32 [count,4], trans f32 [count,3]) on the host.  Every row is a
    function of (seed, step, row) alone, as in augment.sample_params."""
    import numpy as np
    from .augment import _uniforms
    u = _uniforms(int(seed) ^ _RAND_POSE_SALT, int(step), np.arange(count, dtype=np.int64), 6)
    v = (u[:, :3] * 2.0 - 1.0) * 2.5
    theta = np.linalg.norm(v, axis=1, keepdims=True)
    axis = v / np.maximum(theta, 1e-300)
    q = np.concatenate([np.cos(theta / 2), np.sin(theta / 2) * axis], 1)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    return torch.from_numpy(q.astype(np.float32)), torch.from_numpy(((u[:, 3:] - 0.5) * 5.0).astype(np.float32))


def joint_backward(trainers, losses: Dict[str, torch.Tensor], loss_weights: Optional[Dict[str, float]] = None) -> Dict[str, torch.Tensor]:
    """One backward over the sum of `losses` (already weighted, or under `loss_weights`) of a graph that runs through several trainers:
    clears every trainer, differentiates once and returns {state-dict key: gradient} over all of them, each trainer's `.grads` /
    `.input_grads` filled.  The general form of BackboneTrainer.joined_backward."""
    trainers = list(trainers)
    for t in trainers:
        t._clear_grads()
    total = None
    for k, v in losses.items():
        term = v * float(loss_weights.get(k, 1.0)) if loss_weights else v
        total = term if total is None else total + term
    total.backward()
    out: Dict[str, torch.Tensor] = {}
    for t in trainers:
        out.update(t._collect())
    return out


class TwoViewLosses:
    """What siamese_planeTR.py:240-297 adds to the loss dict, from the plane head's outputs of both views: the matching head's embedding
    loss on the matched queries (gathered to a prefix on the device, ops.match_compact) and the camera head's losses with the predicted
    planes on the tape (camera_head_losses(plane_grads=True)) - nothing is detached between the plane head and the two-view heads but
    what the reference detaches.  `camera_head` is the inference head: it supplies the loss weights and switches.

        two_view = TwoViewLosses(matcher, camera, model.camera_head_list[0])
        plane_losses, idx = heads.losses(hs, p1, pair["targets"], groups=2)      # 2B images, view 1 first: the criterion per view
        tv = two_view.losses(hs[-1], heads.last["pred_params"], idx["match_q"][0][:B], idx["match_q"][0][B:], n[:B], n[B:], pair, feats, B)
        grads = joint_backward([heads, matcher, camera], {**heads.criterion.weighted(plane_losses), **tv})"""

    def __init__(self, matcher: "MatchingHeadTrainer", camera: "CameraHeadTrainer", camera_head):
        self.matcher, self.camera, self.camera_head = matcher, camera, camera_head
        self.bad: Optional[torch.Tensor] = None

    def check(self):
        """ValueError if the last losses() call met a match_q / n that breaks match_compact's contract (one host read)."""
        ops.match_compact_check(self.bad)

    def losses(self, query_feat, pred_params, match1, match2, n1, n2, pair: dict, feats: dict, B: int, seed: int = 0, step: int = 0):
        """query_feat [2B,nq,256] (the last layer of hs, view-1 images first), pred_params [2B,nq,3], match1 / match2 int32 [B,nmax] (the
        last layer's match_q of the two views), n1 / n2 int32 [B] on the device, pair = TargetMapper.pair_targets(...), feats = the
        backbone maps -> losses_emb_0 and the camera head's 32 losses (34 with the head's rand_cam_on)."""
        nq, dev = self.matcher.nq, query_feat.device
        _require(query_feat.shape == (2 * B, nq, 256) and pred_params.shape == (2 * B, nq, 3),
                 "TwoViewLosses: query_feat [2B,nq,256], pred_params [2B,nq,3]; got %s, %s" % (tuple(query_feat.shape), tuple(pred_params.shape)))
        n_all = torch.cat([n1, n2]).contiguous()
        x_c, params_c, order, _rank, self.bad = _MatchCompact.apply(query_feat, pred_params, torch.cat([match1, match2]), n_all)
        gt_corr = plane_corr_matrix(pair["gt_corrs"], match1, match2, nq)
        corr_c = ops.corr_compact(gt_corr, order[:B].contiguous(), order[B:].contiguous(), n1.contiguous(), n2.contiguous())
        gt_pose = pair["gt_pose"]
        out = dict(self.matcher.matching_losses(x_c, n_all, gt_pose, params_c[:B], params_c[B:], corr_c, suffix="0"))
        # the camera head: ground-truth planes with the ground-truth correspondences, then all nq predicted planes with gt_corr[:, :nq, :nq]
        t = pair["targets"]
        gt_planes = torch.zeros(2 * B, nq, 3, device=dev, dtype=torch.float32)
        nmax = min(t["plane_params"].shape[1], nq)
        gt_planes[:, :nmax] = t["plane_params"][:, :nmax]
        corrs = pair["gt_corrs"].long()
        valid = (corrs >= 0).all(-1) & (corrs < nq).all(-1)
        flat = (corrs[..., 0].clamp(0, nq - 1) * nq + corrs[..., 1].clamp(0, nq - 1))
        gt_A = torch.zeros(B, nq * nq, device=dev, dtype=torch.float32).scatter_add_(1, flat, valid.float()).clamp_(max=1.0).view(B, nq, nq)
        full = torch.full((B,), nq, device=dev, dtype=torch.int32)
        rand_rot = rand_trans = None
        if getattr(self.camera_head, "rand_cam_on", False):
            rand_rot, rand_trans = (r.to(dev) for r in sample_rand_poses(B * max(1, 64 // B), seed, step))
        out.update(self.camera.camera_head_losses(self.camera_head, feats, B, gt_planes[:B], gt_planes[B:], t["n"][:B].contiguous(),
                                                  t["n"][B:].contiguous(), gt_A, gt_pose, pred_params[:B], pred_params[B:], full, full,
                                                  gt_corr[:, :nq, :nq].float().contiguous(), rand_rot, rand_trans, plane_grads=True))
        return out
