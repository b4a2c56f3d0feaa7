"""utils.seg_helper -- hot-path functions of the reference module, backed by the HIP kernels.

Same names, arguments and error behaviour as the reference (utils/seg_helper.py); every function
cites the lines it replaces.  All tensors live on the GPU; nothing here falls back to the CPU.
"""
import ctypes
import math

import numpy as np
import torch
import torch.nn.functional as F
from torch.autograd import Function

from .. import _C, nn_ops
from ..models.PAR import PAR


def _refresh_once(model):
    """bring the network's 16-bit weight shadows up to date once per multi-scale pass (see nn_ops.ensure_shadows)"""
    f = getattr(getattr(model, "module", model), "refresh_shadows", None)
    if f is not None:
        f()


# --------------------------------------------------------------------------------------------
# multi_scale_camseg  (utils/seg_helper.py:232-275)
# --------------------------------------------------------------------------------------------
def resize_bilinear(x, size):
    """F.interpolate(x, size=size, mode='bilinear', align_corners=False) for NCHW fp32 on the GPU (own kernel: the teacher's input rescale,
    utils/seg_helper.py:247-250, was the last ATen kernel inside the captured teacher pass)"""
    x = x.contiguous().float()
    b, c, h, w = x.shape
    out = torch.empty((b, c, int(size[0]), int(size[1])), device=x.device, dtype=torch.float32)
    _C.check(_C.lib().cosa_resize_bilinear(_C.ptr(x), _C.ptr(out), b * c, h, w, int(size[0]), int(size[1]), _C.stream_ptr()), "cosa_resize_bilinear")
    return out


def _flip_merge_upsample(src, dst, B, S, mode, accumulate, active=None, prev_active=None):
    src = src.contiguous().float()
    _, C, h, w = src.shape
    if prev_active is not None:
        _C.check(_C.lib().cosa_cam_flip_merge_upsample_reuse(_C.ptr(src), _C.ptr(dst), B, C, h, w, S, mode, int(accumulate), _C.ptr(active),
                                                             _C.ptr(prev_active), _C.stream_ptr()), "cosa_cam_flip_merge_upsample_reuse")
        return
    _C.check(_C.lib().cosa_cam_flip_merge_upsample(_C.ptr(src), _C.ptr(dst), B, C, h, w, S, mode, int(accumulate),
                                                   _C.ptr(active), _C.stream_ptr()), "cosa_cam_flip_merge_upsample")


# CAM buffers of a training loop's teacher passes, kept from step to step: a plane that is absent from the image now and was absent
# last time is already zero, so only the planes that were live last time are cleared (80 COCO planes per image, ~3 live: 1 GB of zero
# stores per call otherwise).  The buffers and the `prev` map belong to the CALLER (CoSATrainer passes its own dict as `_buffers`):
# nothing is shared between trainers or with other callers in the process.
def _persistent_cams(store, b, C, h, w, device):
    key = (str(device), b, C, h, w)
    ent = store.get(key)
    if ent is None:
        ent = store[key] = {"cam": torch.zeros((b, C, h, w), device=device, dtype=torch.float32),
                            "aux": torch.zeros((b, C, h, w), device=device, dtype=torch.float32),
                            "prev": torch.zeros((b, C), device=device, dtype=torch.float32)}
    return ent


def cam_minmax_norm_(cam, active=None):
    """In place x -= min; x /= max + 1e-5 per (b,c) plane (utils/seg_helper.py:265-266,269-270)."""
    b, c, h, w = cam.shape
    ws = torch.empty(2 * b * c, device=cam.device, dtype=torch.int32)      # per-plane min / max keys (csrc/label_kernels.hip)
    _C.check(_C.lib().cosa_cam_minmax_norm_ws(_C.ptr(cam), b * c, h * w, _C.ptr(active), _C.ptr(ws), _C.stream_ptr()), "cosa_cam_minmax_norm_ws")
    return cam


def resize_bilinear_f64(x, size):
    """F.interpolate(x.double(), size=size, mode='bilinear', align_corners=False): NCHW fp32 in, float64 planes out (the "fp64" mode's input rescale)"""
    x = x.contiguous().float()
    b, c, h, w = x.shape
    out = torch.empty((b, c, int(size[0]), int(size[1])), device=x.device, dtype=torch.float64)
    _C.check(_C.lib().cosa_resize_bilinear_f64(_C.ptr(x), _C.ptr(out), b * c, h, w, int(size[0]), int(size[1]), _C.stream_ptr()),
             "cosa_resize_bilinear_f64")
    return out


def _flip_merge_upsample_f64(src, dst, B, S, mode, accumulate, active=None, rawmax=None):
    """the float64 tail kernel: src [2B, C, h, w] float64 -> dst [B, C, S, S] float64 (+= with accumulate); rawmax [B, C] float64 or None:
    (+)= per plane max |src| over the plane and its mirror image's plane"""
    assert src.dtype == torch.float64 and dst.dtype == torch.float64 and dst.is_contiguous() and (rawmax is None or rawmax.dtype == torch.float64)
    src = src.contiguous()
    _, C, h, w = src.shape
    _C.check(_C.lib().cosa_cam_flip_merge_upsample_f64(_C.ptr(src), _C.ptr(dst), B, C, h, w, S, mode, int(accumulate), _C.ptr(active),
                                                       _C.ptr(rawmax), _C.stream_ptr()), "cosa_cam_flip_merge_upsample_f64")


def cam_minmax_norm_f64_(cam, active=None, peak=None):
    """cam_minmax_norm_ on float64 planes, in place; peak [b, c] float64 or None: what each live plane was divided by (max of plane - min, + 1e-5)"""
    assert cam.dtype == torch.float64 and cam.is_contiguous() and (peak is None or (peak.dtype == torch.float64 and peak.is_contiguous()))
    b, c, h, w = cam.shape
    _C.check(_C.lib().cosa_cam_minmax_norm_f64(_C.ptr(cam), b * c, h * w, _C.ptr(active), _C.ptr(peak), _C.stream_ptr()), "cosa_cam_minmax_norm_f64")
    return cam


def _is_f64_model(model):
    return getattr(getattr(getattr(model, "module", model), "encoder", None), "precision", None) == "f64"


def _multi_scale_camseg_f64(model, imgs, scales, act, seg_scales, return_scale):
    """multi_scale_camseg for a network in mode "fp64": float64 from the input rescale to the normalised CAM.  -> float64 cam, cam_aux, seg
    (or the per-scale float64 seg list) and, with return_scale, ((peak, rawmax) of cam, (peak, rawmax) of cam_aux), each [b, C] float64: peak =
    max of the un-normalised plane minus its minimum, + 1e-5 (what the normalisation divides by); rawmax = the sum over the scales of max |class
    logit| over the plane and its mirror image's (the last scale alone for cam_aux) -- the test-suite's CPU restatement defines them the same way"""
    b, c, h, w = imgs.shape
    dev = imgs.device
    seg_list = []
    with torch.no_grad():
        scaled = [imgs.double() if s == 1.0 else resize_bilinear_f64(imgs, (int(s * h), int(s * w))) for s in scales]
        if not model.can_forward_multi(scaled[0]):
            raise _C.CosaError("multi_scale_camseg: the fp64 mode runs on the fused no-grad HIP path only")
        multi = model.forward_multi(scaled, flip_pairs=True, need_cls=False)
        C, K = multi[0][4].shape[1], multi[0][3].shape[1]
        z = lambda *shape: torch.zeros(shape, device=dev, dtype=torch.float64)
        cam, cam_aux, seg = z(b, C, h, w), z(b, C, h, w), (None if seg_scales else z(b, K, h, w))
        peak, rawmax, peak_aux, rawmax_aux = z(b, C), z(b, C), z(b, C), z(b, C)
        for si in range(len(scales)):
            _, _, _, _seg, _cam, _cam_aux = multi[si]
            _flip_merge_upsample_f64(_cam, cam, b, h, 0, si > 0, act, rawmax)
            if si == len(scales) - 1:                                   # only the last scale survives (:258)
                _flip_merge_upsample_f64(_cam_aux, cam_aux, b, h, 0, False, act, rawmax_aux)
            if seg_scales:
                seg_list.append(_seg.contiguous())
            else:
                _flip_merge_upsample_f64(_seg, seg, b, h, 1, si > 0)
        cam_minmax_norm_f64_(cam, act, peak)
        cam_minmax_norm_f64_(cam_aux, act, peak_aux)
    out = (cam, cam_aux, seg_list if seg_scales else seg)
    return out + ((peak, rawmax), (peak_aux, rawmax_aux)) if return_scale else out


def multi_scale_camseg(model, imgs, scales, _active_labels=None, _seg_scales=False, _buffers=None, _return_scale=False):
    """Teacher forward over scales x {orig, flip}; returns (cam, cam_aux, seg) at input size.

    utils/seg_helper.py:232-275.  Per scale one fused kernel does bilinear-up + un-flip + max/sum
    (+ReLU) + accumulation; the reference's quirk that cam_aux keeps ONLY the last scale
    (`cam_aux_list = [...]`, :258) is reproduced.  `_active_labels` ([b,C] image-level labels, optional): the CAM
    planes of absent classes are returned as zeros -- exactly what cam_validation makes of them in the very next
    call of the training loop (main.py:137) -- so the tail only touches the 1-4 live planes per image.
    `_seg_scales=True` returns the per-scale low-res seg outputs (a list of [2b,K,h_s,w_s]) in place of the summed
    full-resolution seg: the only consumer in the loop (cam_loss's targets) reads 4 pixels per 16x16 block of it
    (see cam_loss_targets), so the [b,K,S,S] tensor need not exist.
    `_buffers` (a dict owned by the caller, with `_active_labels` only): the returned cam / cam_aux then live in buffers kept in that dict
    from call to call (planes absent now and last time are not re-zeroed) -- they are VALID ONLY UNTIL THE NEXT CALL with the same dict
    and shapes, and must not be written in place by the caller.  Without it every call returns fresh tensors.
    A network in mode "fp64"  runs the float64 tail and returns float64 tensors, always fresh ones; `_return_scale=True`
    (that mode only) appends ((peak, rawmax) of cam, (peak, rawmax) of cam_aux), [b, C] float64 each.
    """
    b, c, h, w = imgs.shape
    assert 1.0 in scales, 'scale 1.0 must be in scales'
    assert h == w, "square crops only"
    _C.require_cuda(imgs)
    if _is_f64_model(model):
        act64 = _active_labels.contiguous().float() if _active_labels is not None else None
        return _multi_scale_camseg_f64(model, imgs, scales, act64, _seg_scales, _return_scale)
    if _return_scale:
        raise ValueError("multi_scale_camseg: _return_scale needs a network in mode 'fp64' (the scale figures come from the float64 pass)")
    cam = cam_aux = seg = None
    seg_list = []
    act = _active_labels.contiguous().float() if _active_labels is not None else None
    with torch.no_grad():
        scaled = [imgs if s == 1.0 else resize_bilinear(imgs, (int(s * h), int(s * w))) for s in scales]
        # cosa_amd networks can take all scales in one go (shared GEMM/LayerNorm launches across scales), the mirror images only as
        # im2col rows of the patch projection (flip_pairs)
        if getattr(model, "can_forward_multi", lambda _x: False)(scaled[0]):
            multi, inputs = model.forward_multi(scaled, flip_pairs=True, need_cls=False), None
        else:
            multi, inputs = None, [torch.cat([x_, x_.flip(-1)], dim=0) for x_ in scaled]
            _refresh_once(model)
        for si, s in enumerate(scales):
            with nn_ops.shadows_fresh(model):
                _, _, _, _seg, _cam, _cam_aux = multi[si] if multi is not None else model(inputs[si], cam_only=False)
            if cam is None:
                if act is not None and _buffers is not None:
                    keep = _persistent_cams(_buffers, b, _cam.shape[1], h, w, imgs.device)
                    cam, cam_aux, prev = keep["cam"], keep["aux"], keep["prev"]
                elif act is not None:
                    cam = torch.zeros((b, _cam.shape[1], h, w), device=imgs.device, dtype=torch.float32)
                    cam_aux = torch.zeros_like(cam)
                    prev = torch.zeros((b, _cam.shape[1]), device=imgs.device, dtype=torch.float32)
                else:
                    cam = torch.empty((b, _cam.shape[1], h, w), device=imgs.device, dtype=torch.float32)
                    cam_aux = torch.empty_like(cam)
                    prev = None
                seg = None if _seg_scales else torch.empty((b, _seg.shape[1], h, w), device=imgs.device, dtype=torch.float32)
            _flip_merge_upsample(_cam, cam, b, h, 0, si > 0, act, prev if si == 0 else None)
            if si == len(scales) - 1:                                   # only the last scale survives (:258)
                _flip_merge_upsample(_cam_aux, cam_aux, b, h, 0, False, act, prev)
            if _seg_scales:
                seg_list.append(_seg.contiguous().float())
            else:
                _flip_merge_upsample(_seg, seg, b, h, 1, si > 0)
        cam_minmax_norm_(cam, act)
        cam_minmax_norm_(cam_aux, act)
        if act is not None:
            prev.copy_(act.view_as(prev))
    return cam, cam_aux, (seg_list if _seg_scales else seg)


def multi_scale_camsegv3(model, imgs, scales, getcls=False, _per_image_cls=False):
    """Evaluation-time variant (utils/seg_helper.py:399-450; evaluation_engine.py:82-85 calls it with five scales x two flips):
    same fused tail as multi_scale_camseg, plus the classification logits summed over scales and over {orig, flip}
    (`cls_f_ += sum(cls_f, dim=0)`, :432-434).  cam_aux again keeps only the LAST scale (:426)."""
    b, c, h, w = imgs.shape
    assert 1.0 in scales, 'scale 1.0 must be in scales'
    assert h == w, "square inputs only (evaluation resizes to crop_size x crop_size first)"
    _C.require_cuda(imgs)
    cam = cam_aux = seg = None
    cls_f_ = cls_a_ = None
    with torch.no_grad():
        scaled = [imgs if s == 1.0 else resize_bilinear(imgs, (int(s * h), int(s * w))) for s in scales]
        if getattr(model, "can_forward_multi", lambda _x: False)(scaled[0]):
            multi, inputs = model.forward_multi(scaled, flip_pairs=True, need_cls=bool(getcls)), None
        else:
            multi, inputs = None, [torch.cat([x_, x_.flip(-1)], dim=0) for x_ in scaled]
            _refresh_once(model)
        for si, s in enumerate(scales):
            with nn_ops.shadows_fresh(model):
                cls_f, cls_a, _, _seg, _cam, _cam_aux = multi[si] if multi is not None else model(inputs[si], cam_only=False)
            if cam is None:
                cam = torch.empty((b, _cam.shape[1], h, w), device=imgs.device, dtype=torch.float32)
                cam_aux = torch.empty_like(cam)
                seg = torch.empty((b, _seg.shape[1], h, w), device=imgs.device, dtype=torch.float32)
            _flip_merge_upsample(_cam, cam, b, h, 0, si > 0)
            if si == len(scales) - 1:
                _flip_merge_upsample(_cam_aux, cam_aux, b, h, 0, False)
            _flip_merge_upsample(_seg, seg, b, h, 1, si > 0)
            if getcls and _per_image_cls:
                # several images per pass (evaluate's grouping): the reference's sum over {orig, flip} kept per image -> [b, C]
                cf, ca = cls_f.float().reshape(2, b, -1).sum(0), cls_a.float().reshape(2, b, -1).sum(0)
                cls_f_ = cf if cls_f_ is None else cls_f_ + cf
                cls_a_ = ca if cls_a_ is None else cls_a_ + ca
            elif getcls:
                cf, ca = cls_f.float().sum(0, keepdim=True), cls_a.float().sum(0, keepdim=True)
                cls_f_ = cf if cls_f_ is None else cls_f_ + cf
                cls_a_ = ca if cls_a_ is None else cls_a_ + ca
        cam_minmax_norm_(cam)
        cam_minmax_norm_(cam_aux)
    if getcls:
        return cam, cam_aux, seg, cls_f_, cls_a_
    return cam, cam_aux, seg


# --------------------------------------------------------------------------------------------
# cam_to_label / seg_validation / evaluation label maps  (utils/seg_helper.py:515-546, 581-591; evaluation_engine.py:96-126,198-200)
# --------------------------------------------------------------------------------------------
def cam_to_label(cam, cls_label, img_box=None, bkg_thre=None, high_thre=None, low_thre=None, ignore_mid=False, ignore_index=None):
    """utils/seg_helper.py:515-546: argmax of the class-validated CAM (+1), background where the max <= bkg_thre.
    Returns the int64 label map when `img_box` is None, else `(valid_cam, pseudo_label)` with the label confined to the boxes
    (ignore_index outside) and, if `ignore_mid`, the high/low threshold band marked ignore_index."""
    _C.require_cuda(cam)
    if bkg_thre is None:
        raise TypeError("cam_to_label: bkg_thre is required (the reference compares against it unconditionally)")
    cam = cam.contiguous().float()
    b, c, h, w = cam.shape
    cls = cls_label.contiguous().float() if cls_label is not None else None
    label = torch.empty((b, h, w), device=cam.device, dtype=torch.int64)
    boxes = valid = None
    if img_box is not None:
        boxes = _boxes_to_device(img_box, cam.device)
        if boxes.shape != (b, 4):
            raise ValueError("cam_to_label: img_box must be [b,4]")
        if ignore_index is None or (ignore_mid and (high_thre is None or low_thre is None)):
            raise TypeError("cam_to_label: ignore_index (and high_thre/low_thre with ignore_mid) are required with img_box")
        valid = torch.empty_like(cam)
    _C.check(_C.lib().cosa_cam_to_label(_C.ptr(cam), _C.ptr(cls), b, c, h, w, float(bkg_thre), _C.ptr(boxes), int(bool(ignore_mid)),
                                        float(high_thre or 0.0), float(low_thre or 0.0), int(ignore_index if ignore_index is not None else 255),
                                        _C.ptr(label), _C.ptr(valid), _C.stream_ptr()), "cosa_cam_to_label")
    return label if img_box is None else (valid, label)


def seg_validation(seg, cls_label):
    """utils/seg_helper.py:581-591: logits of the classes absent from the image-level label set to -1e5 (background kept)."""
    if cls_label is None:
        return seg
    b = seg.shape[0]
    present = torch.cat([torch.ones(b, 1, device=seg.device, dtype=torch.bool), cls_label != 0], dim=1)
    return torch.where(present[:, :, None, None], seg, torch.full((), -1e5, device=seg.device, dtype=seg.dtype))


def eval_label_maps(cam, seg, cls_label, size, bkg_thre):
    """One launch for evaluation_engine.py:96-126,198-200: `F.interpolate(cam, size)` -> cam_to_label(bkg_thre),
    `F.interpolate(seg, size)` -> argmax, seg_validation -> argmax, without the resized tensors.
    cam [b,C,S,S] and/or seg [b,C+1,S,S] -> uint8 maps [b,H,W]: (cam_label, pred_ps, pred_vd) (None for an absent input)."""
    H, W = int(size[0]), int(size[1])
    ref = cam if cam is not None else seg
    _C.require_cuda(ref, cls_label)
    b, S = ref.shape[0], ref.shape[-1]
    C = cls_label.shape[1]
    cam = cam.contiguous().float() if cam is not None else None
    seg = seg.contiguous().float() if seg is not None else None
    if (cam is not None and cam.shape != (b, C, S, S)) or (seg is not None and seg.shape != (b, C + 1, S, S)):
        raise ValueError("eval_label_maps: cam must be [b,C,S,S] and seg [b,C+1,S,S]")
    mk = lambda: torch.empty((b, H, W), device=ref.device, dtype=torch.uint8)
    lc = mk() if cam is not None else None
    lp, lv = (mk(), mk()) if seg is not None else (None, None)
    _C.check(_C.lib().cosa_eval_labels(_C.ptr(cam), _C.ptr(seg), _C.ptr(cls_label.contiguous().float()), b, C, S, H, W, float(bkg_thre),
                                       _C.ptr(lc), _C.ptr(lp), _C.ptr(lv), _C.stream_ptr()), "cosa_eval_labels")
    return lc, lp, lv


# --------------------------------------------------------------------------------------------
# the monitors' counter vectors: each C layout function is THE definition of its vector, the lengths here come from it
# --------------------------------------------------------------------------------------------
def _c_layout(fn, slots, K):
    """a C layout function's answer as ({slot name: offset in elements}, number of elements)"""
    off = (ctypes.c_size_t * len(slots))()
    n = fn(int(K), off)
    if n == 0:
        raise ValueError(_C.lib().cosa_last_error().decode("utf-8", "replace"))
    return {name: int(off[i]) for i, name in enumerate(slots)}, int(n)


def _new_counters(layout, device):
    """a zeroed counter vector of `layout`'s length (int64: the uint64 counters of the C ABI, which stay below 2^63)"""
    return torch.zeros(layout[1], dtype=torch.int64, device=device)


def _check_counters(counters, layout, who):
    """`counters` is a contiguous int64 vector of `layout`'s length, as new_<who> makes it"""
    n = layout[1]
    if counters.dtype != torch.int64 or counters.shape != (n,) or not counters.is_contiguous():
        raise ValueError(f"{who}: counters must be a contiguous int64 vector of {n} elements (new_{who})")


# --------------------------------------------------------------------------------------------
# per-step pseudo-label statistics and the teacher finite check
# --------------------------------------------------------------------------------------------
LABEL_STATS_SLOTS = ("steps", "pix", "main", "aux", "agree", "inter", "pred", "bad_cam", "bad_cam_aux")     # cosa_label_stats_layout's order
assert len(LABEL_STATS_SLOTS) == _C.constant("COSA_LABEL_STATS_SLOTS")
LABEL_STATS_MAX_K = 128


def label_stats_layout(K):
    """cosa_label_stats_layout: ({slot name: offset in elements}, number of elements) of the counter vector for K = num_classes
    (background included).  Needs no device."""
    return _c_layout(_C.lib().cosa_label_stats_layout, LABEL_STATS_SLOTS, K)


def new_label_stats(K, device):
    """a zeroed counter vector (int64: the uint64 counters of the C ABI, which stay far below 2^63)"""
    return _new_counters(label_stats_layout(K), device)


def _label_stats_shapes(mask_main, mask_aux, seg_logits, cls_label, cam, cam_aux, counters):
    B, S = mask_main.shape[0], mask_main.shape[-1]
    K = seg_logits.shape[1]
    h, w = seg_logits.shape[-2:]
    if mask_main.shape != (B, S, S) or (mask_aux is not None and mask_aux.shape != (B, S, S)) or seg_logits.shape != (B, K, h, w) or \
            cls_label.shape != (B, K - 1) or any(c is not None and c.shape != (B, K - 1, S, S) for c in (cam, cam_aux)):
        raise ValueError("label_stats: masks must be [B,S,S], seg_logits [B,K,h,w], cls_label [B,K-1] and the CAMs [B,K-1,S,S]")
    _check_counters(counters, label_stats_layout(K), "label_stats")
    return B, K, S, int(h), int(w)


def label_stats(mask_main, mask_aux, seg_logits, cls_label, img_box, cam, cam_aux, counters, ignore_index=255, step_scale=None):
    """One reduction (cosa_label_stats) over what a training step holds anyway, accumulated into `counters` on the device: label-map
    histograms of the main and auxiliary pseudo labels inside the crop boxes, their agreement, the per-class intersection / count of
    the student's own segmentation against the main labels, and the non-finite elements of the present classes' CAM planes.
    mask_aux, cam, cam_aux may be None.  -> step_scale, a one-element fp32 device tensor: 1.0 when this call met only finite CAMs,
    NaN otherwise.  No host sync."""
    _C.require_cuda(mask_main, mask_aux, seg_logits, cls_label, cam, cam_aux, counters)
    f = lambda t: t.detach().contiguous().float() if t is not None else None
    mask_main, mask_aux, seg_logits, cls_label, cam, cam_aux = (f(t) for t in (mask_main, mask_aux, seg_logits, cls_label, cam, cam_aux))
    B, K, S, h, w = _label_stats_shapes(mask_main, mask_aux, seg_logits, cls_label, cam, cam_aux, counters)
    dev = mask_main.device
    boxes = _boxes_to_device(img_box, dev)
    if step_scale is None:
        step_scale = torch.empty(1, device=dev, dtype=torch.float32)
    ws = _C.workspace(_C.constant("COSA_LABEL_STATS_WORKSPACE_BYTES"), dev, "label_stats")
    _C.check(_C.lib().cosa_label_stats(_C.ptr(mask_main), _C.ptr(mask_aux), _C.ptr(seg_logits), _C.ptr(cls_label), _C.ptr(boxes), _C.ptr(cam),
                                       _C.ptr(cam_aux), B, K, S, h, w, int(ignore_index), _C.ptr(counters), _C.ptr(step_scale), _C.ptr(ws),
                                       _C.stream_ptr()), "cosa_label_stats")
    return step_scale


@torch.no_grad()
def label_stats_torch(mask_main, mask_aux, seg_logits, cls_label, img_box, cam, cam_aux, counters, ignore_index=255, step_scale=None):
    """label_stats in plain torch, for host trainers (the role guarded_torch_step plays for the gradient guard): F.interpolate + argmax
    instead of the kernel's spec-R resize, the same counters in the same layout."""
    f = lambda t: t.detach().float() if t is not None else None
    mask_main, mask_aux, seg_logits, cls_label, cam, cam_aux = (f(t) for t in (mask_main, mask_aux, seg_logits, cls_label, cam, cam_aux))
    B, K, S, h, w = _label_stats_shapes(mask_main, mask_aux, seg_logits, cls_label, cam, cam_aux, counters)
    if K > LABEL_STATS_MAX_K or h > S or w > S or 0 <= int(ignore_index) < K:
        raise ValueError(f"label_stats: outside the envelope (K {K} <= {LABEL_STATS_MAX_K}, h {h} and w {w} <= S {S}, ignore_index no class)")
    dev = mask_main.device
    off, _ = label_stats_layout(K)
    box = torch.as_tensor(img_box).to(device=dev, dtype=torch.int64)
    ar = torch.arange(S, device=dev)
    inside = ((ar[None, :, None] >= box[:, 0, None, None]) & (ar[None, :, None] < box[:, 1, None, None]) &
              (ar[None, None, :] >= box[:, 2, None, None]) & (ar[None, None, :] < box[:, 3, None, None]))
    add = torch.zeros_like(counters)
    add[off["steps"]] = 1
    add[off["pix"]] = inside.sum()

    def hist(mask, valid):
        """[K+1] counts of the values 0..K-1 and (slot K) ignore_index"""
        slot = torch.where(mask == ignore_index, torch.full_like(mask, K), mask)
        ok = valid & (slot >= 0) & (slot <= K) & (slot == slot.floor())          # a value that is no label is not counted
        return torch.bincount(slot[ok].long(), minlength=K + 1)

    add[off["main"]:off["main"] + K + 1] = hist(mask_main, inside)
    if mask_aux is not None:
        add[off["aux"]:off["aux"] + K + 1] = hist(mask_aux, inside)
        add[off["agree"]] = (inside & (mask_main == mask_aux)).sum()
    student = seg_validation(F.interpolate(seg_logits, size=(S, S), mode="bilinear", align_corners=False), cls_label).argmax(dim=1)
    labelled = inside & (mask_main >= 0) & (mask_main < K) & (mask_main == mask_main.floor())
    add[off["pred"]:off["pred"] + K] = torch.bincount(student[labelled], minlength=K)
    add[off["inter"]:off["inter"] + K] = torch.bincount(student[labelled & (student == mask_main.long())], minlength=K)
    bad = torch.zeros((), dtype=torch.int64, device=dev)
    for name, c in (("bad_cam", cam), ("bad_cam_aux", cam_aux)):
        if c is not None:
            n = (~torch.isfinite(c) & (cls_label != 0)[:, :, None, None] & inside[:, None]).sum()
            add[off[name]] = n
            bad = bad + n
    counters += add
    if step_scale is None:
        step_scale = torch.empty(1, device=dev, dtype=torch.float32)
    step_scale.copy_(torch.where(bad > 0, torch.full((), float("nan"), device=dev), torch.ones((), device=dev)).reshape(1))
    return step_scale


def label_stats_summary(counters, K):
    """The counter vector (tensor, array or list; a device tensor synchronises) as the figures a log line shows: ignore / background /
    foreground fractions of the main and auxiliary label maps inside the boxes, the share of pixels where the two agree, the student's
    mIoU against the main labels (mean of inter / (pred + main - inter) over the classes with a non-zero union) with the per-class
    list (None for an empty union), the non-finite CAM elements met, and the steps accumulated.  Zero pixels give zeros, not NaN."""
    c = [int(v) for v in (counters.tolist() if hasattr(counters, "tolist") else counters)]
    off, n = label_stats_layout(K)
    if len(c) != n:
        raise ValueError(f"label_stats_summary: {len(c)} counters, K = {K} has {n}")
    pix = c[off["pix"]]
    frac = lambda v: v / pix if pix else 0.0
    out = {"steps": c[off["steps"]], "pix": pix}
    for tag, name in (("", "main"), ("aux_", "aux")):
        hist = c[off[name]:off[name] + K + 1]
        out[tag + "ignore_frac"], out[tag + "bg_frac"], out[tag + "fg_frac"] = frac(hist[K]), frac(hist[0]), frac(sum(hist[1:K]))
        out[tag + "class_pixels"] = hist
    out["aux_agree"] = frac(c[off["agree"]])
    main = c[off["main"]:off["main"] + K]
    inter, pred = c[off["inter"]:off["inter"] + K], c[off["pred"]:off["pred"] + K]
    union = [p + m - i for p, m, i in zip(pred, main, inter)]
    iou = [i / u if u else None for i, u in zip(inter, union)]
    live = [v for v in iou if v is not None]
    out["student_iou"] = iou
    out["student_miou"] = sum(live) / len(live) if live else 0.0
    out["teacher_nonfinite"] = c[off["bad_cam"]] + c[off["bad_cam_aux"]]
    out["teacher_nonfinite_main"], out["teacher_nonfinite_aux"] = c[off["bad_cam"]], c[off["bad_cam_aux"]]
    return out


# --------------------------------------------------------------------------------------------
# --gt_stats: pseudo labels and the student's prediction against the ground truth of the training crops
# --------------------------------------------------------------------------------------------
GT_STATS_SLOTS = ("steps", "pix", "valid", "gt_other", "main", "aux", "student")     # cosa_gt_stats_layout's order
assert len(GT_STATS_SLOTS) == _C.constant("COSA_GT_STATS_SLOTS")


def gt_stats_layout(K):
    """cosa_gt_stats_layout: ({slot name: offset in elements}, number of elements) of the counter vector for K = num_classes (background
    included): steps, pix, valid, gt_other, main[K][K+1], aux[K][K+1], student[K][K] (row: the ground-truth class; column K of main and
    aux: the label map's ignore).  Needs no device."""
    return _c_layout(_C.lib().cosa_gt_stats_layout, GT_STATS_SLOTS, K)


def new_gt_stats(K, device):
    """a zeroed counter vector (int64: the uint64 counters of the C ABI, which stay far below 2^63)"""
    return _new_counters(gt_stats_layout(K), device)


def _gt_stats_shapes(gt, mask_main, mask_aux, seg_logits, cls_label, counters):
    B, S = mask_main.shape[0], mask_main.shape[-1]
    K = seg_logits.shape[1]
    h, w = seg_logits.shape[-2:]
    if gt.dtype != torch.uint8 or gt.shape != (B, S, S) or mask_main.shape != (B, S, S) or \
            (mask_aux is not None and mask_aux.shape != (B, S, S)) or seg_logits.shape != (B, K, h, w) or cls_label.shape != (B, K - 1):
        raise ValueError("gt_stats: gt must be uint8 [B,S,S], the masks [B,S,S], seg_logits [B,K,h,w] and cls_label [B,K-1]")
    _check_counters(counters, gt_stats_layout(K), "gt_stats")
    return B, K, S, int(h), int(w)


def gt_stats(gt, mask_main, mask_aux, seg_logits, cls_label, img_box, counters, ignore_index=255):
    """One reduction (cosa_gt_stats) accumulated into `counters` on the device: the confusion matrices of the main label map, the
    auxiliary one (may be None: its block stays as it is) and the student's own segmentation against the ground-truth crop `gt`
    (uint8 [B,S,S], 255 = no ground truth), over the pixels inside the crop boxes whose ground truth is a class.  No host sync."""
    _C.require_cuda(gt, mask_main, mask_aux, seg_logits, cls_label, counters)
    f = lambda t: t.detach().contiguous().float() if t is not None else None
    mask_main, mask_aux, seg_logits, cls_label = (f(t) for t in (mask_main, mask_aux, seg_logits, cls_label))
    gt = gt.contiguous()
    B, K, S, h, w = _gt_stats_shapes(gt, mask_main, mask_aux, seg_logits, cls_label, counters)
    boxes = _boxes_to_device(img_box, mask_main.device)
    _C.check(_C.lib().cosa_gt_stats(_C.ptr(gt), _C.ptr(mask_main), _C.ptr(mask_aux), _C.ptr(seg_logits), _C.ptr(cls_label), _C.ptr(boxes),
                                    B, K, S, h, w, int(ignore_index), _C.ptr(counters), _C.stream_ptr()), "cosa_gt_stats")


@torch.no_grad()
def gt_stats_torch(gt, mask_main, mask_aux, seg_logits, cls_label, img_box, counters, ignore_index=255):
    """gt_stats in plain torch, for host trainers (the role label_stats_torch plays): F.interpolate + argmax instead of the kernel's
    spec-R resize (torch's argmax takes the first maximum, as the kernel does), the same counters in the same layout."""
    f = lambda t: t.detach().float() if t is not None else None
    mask_main, mask_aux, seg_logits, cls_label = (f(t) for t in (mask_main, mask_aux, seg_logits, cls_label))
    B, K, S, h, w = _gt_stats_shapes(gt, mask_main, mask_aux, seg_logits, cls_label, counters)
    if K > LABEL_STATS_MAX_K or h > S or w > S or 0 <= int(ignore_index) < K:
        raise ValueError(f"gt_stats: outside the envelope (K {K} <= {LABEL_STATS_MAX_K}, h {h} and w {w} <= S {S}, ignore_index no class)")
    dev = mask_main.device
    off, _ = gt_stats_layout(K)
    box = torch.as_tensor(img_box).to(device=dev, dtype=torch.int64)
    ar = torch.arange(S, device=dev)
    inside = ((ar[None, :, None] >= box[:, 0, None, None]) & (ar[None, :, None] < box[:, 1, None, None]) &
              (ar[None, None, :] >= box[:, 2, None, None]) & (ar[None, None, :] < box[:, 3, None, None]))
    g = gt.to(dev).long()
    valid = inside & (g < K)
    add = torch.zeros_like(counters)
    add[off["steps"]] = 1
    add[off["pix"]] = inside.sum()
    add[off["valid"]] = valid.sum()
    add[off["gt_other"]] = (inside & (g >= K) & (g != 255)).sum()
    for name, mask in (("main", mask_main), ("aux", mask_aux)):
        if mask is None:
            continue
        slot = torch.where(mask == ignore_index, torch.full_like(mask, K), mask)
        ok = valid & (slot >= 0) & (slot <= K) & (slot == slot.floor())          # a value that is no label is not counted
        add[off[name]:off[name] + K * (K + 1)] = torch.bincount(g[ok] * (K + 1) + slot[ok].long(), minlength=K * (K + 1))
    student = seg_validation(F.interpolate(seg_logits, size=(S, S), mode="bilinear", align_corners=False), cls_label).argmax(dim=1)
    add[off["student"]:off["student"] + K * K] = torch.bincount(g[valid] * K + student[valid], minlength=K * K)
    counters += add


def _iou_rows(mat, K, cols, strict_col=None):
    """per-class IoU of a [K][cols] confusion matrix (row: ground truth) over its first K columns: inter / (row + column - inter); with
    strict_col the pixels of that column (the label map's ignore) stay in their ground-truth class's union and in no intersection.  An
    empty union gives None.  -> (iou[K], mean over the classes with a union, 0.0 when there is none)"""
    iou = []
    for k in range(K):
        inter = mat[k * cols + k]
        row = sum(mat[k * cols + c] for c in range(K)) + (mat[k * cols + strict_col] if strict_col is not None else 0)
        col = sum(mat[t * cols + k] for t in range(K))
        union = row + col - inter
        iou.append(inter / union if union else None)
    live = [v for v in iou if v is not None]
    return iou, (sum(live) / len(live) if live else 0.0)


def gt_stats_summary(counters, K):
    """The counter vector (tensor, array or list; a device tensor synchronises) as figures: steps, pix, valid_frac (valid / pix) and
    gt_other at the top; for `main` and `aux` the share of valid pixels that carry a label (`labelled`), `miou` / `iou[K]` from the
    confusion matrix with the ignore column dropped (the quality of the labels that exist), and `miou_strict` / `iou_strict[K]`, where an
    ignore pixel is a miss: in its ground-truth class's union, in no intersection (quality times coverage); for `student` `miou` and
    `iou[K]`.  A class with an empty union is None and stays out of its mean; all-zero counters give zeros, not NaN."""
    c = [int(v) for v in (counters.tolist() if hasattr(counters, "tolist") else counters)]
    off, n = gt_stats_layout(K)
    if len(c) != n:
        raise ValueError(f"gt_stats_summary: {len(c)} counters, K = {K} has {n}")
    pix, valid = c[off["pix"]], c[off["valid"]]
    out = {"steps": c[off["steps"]], "pix": pix, "valid_frac": valid / pix if pix else 0.0, "gt_other": c[off["gt_other"]]}
    for name in ("main", "aux"):
        mat = c[off[name]:off[name] + K * (K + 1)]
        total, ign = sum(mat), sum(mat[k * (K + 1) + K] for k in range(K))
        iou, miou = _iou_rows(mat, K, K + 1)
        iou_s, miou_s = _iou_rows(mat, K, K + 1, strict_col=K)
        out[name] = {"labelled": (total - ign) / valid if valid else 0.0, "miou": miou, "iou": iou, "miou_strict": miou_s, "iou_strict": iou_s,
                     "pixels": total}
    iou, miou = _iou_rows(c[off["student"]:off["student"] + K * K], K, K)
    out["student"] = {"miou": miou, "iou": iou}
    return out


# --------------------------------------------------------------------------------------------
# the --teacher_check monitor: two teacher passes on two operand modes, scored against each other
# --------------------------------------------------------------------------------------------
TEACHER_CHECK_SETS = ("cam", "aux", "tgt")                       # map sets, then label pairs: cosa_teacher_check_layout's order
TEACHER_CHECK_PAIRS = ("main", "aux_label")
_TC_SET_FIELDS = ("planes", "over", "worst", "hist", "nonfinite_a", "nonfinite_b")
_TC_PAIR_FIELDS = ("pix", "agree", "ign_a", "ign_b", "cnt_a", "cnt_b", "inter")
TEACHER_CHECK_SLOTS = ("checks",) + tuple(f"{s}.{f}" for s in TEACHER_CHECK_SETS for f in _TC_SET_FIELDS) + \
    tuple(f"{p}.{f}" for p in TEACHER_CHECK_PAIRS for f in _TC_PAIR_FIELDS)
assert len(TEACHER_CHECK_SLOTS) == _C.constant("COSA_TEACHER_CHECK_SLOTS")
TEACHER_CHECK_EDGES = (1e-6, 1e-5, 1e-4, 3e-4, 1e-3, 3e-3, 1e-2, float("inf"))      # upper edges of hist (as fp32), a plane in the first bin with fig <= edge
TEACHER_CHECK_BAR = 1e-3                                          # the literal bar of tests/test_precision_gpu.py: normalised-CAM |delta| per plane
TEACHER_CHECK_AGREE, TEACHER_CHECK_MIOU = 0.999, 0.999            # ... its label agreement and mask mIoU
TEACHER_CHECK_MAX_K = 256


def teacher_check_layout(K):
    """cosa_teacher_check_layout: ({slot name: offset in elements}, number of elements) of the counter vector for K = num_classes
    (background included).  Slot names are "checks", "<set>.<field>" for the map sets cam / aux / tgt and "<pair>.<field>" for the label
    pairs main / aux_label.  Needs no device."""
    return _c_layout(_C.lib().cosa_teacher_check_layout, TEACHER_CHECK_SLOTS, K)


def new_teacher_check(K, device):
    """a zeroed counter vector (int64: the uint64 counters of the C ABI, which stay far below 2^63)"""
    return _new_counters(teacher_check_layout(K), device)


def _teacher_check_shapes(cams, auxs, tgts, labels, aux_labels, cls_label, counters):
    B, C, S = cams[0].shape[0], cams[0].shape[1], cams[0].shape[-1]
    h = w = 0
    ok = all(t.shape == (B, C, S, S) for t in tuple(cams) + tuple(auxs)) and all(t.shape == (B, S, S) for t in labels)
    if tgts is not None:
        h, w = (int(v) for v in tgts[0].shape[-2:])
        ok = ok and all(t.shape == (B, C, h, w) for t in tgts)
    if aux_labels is not None:
        ok = ok and all(t.shape == (B, S, S) for t in aux_labels)
    if cls_label is not None:
        ok = ok and cls_label.shape == (B, C)
    if not ok:
        raise ValueError("teacher_check: CAM pairs must be [B,C,S,S], the target pair [B,C,h,w], label maps [B,S,S] and cls_label [B,C]")
    K = C + 1
    if K > TEACHER_CHECK_MAX_K or h > S or w > S:
        raise ValueError(f"teacher_check: outside the envelope (C {C} <= {TEACHER_CHECK_MAX_K - 1}, h {h} and w {w} <= S {S})")
    _check_counters(counters, teacher_check_layout(K), "teacher_check")
    return B, C, K, S, h, w


def teacher_check(cams, auxs, tgts, labels, aux_labels, cls_label, img_box, counters, ignore_index=255, bar=TEACHER_CHECK_BAR):
    """One reduction (cosa_teacher_check) that scores two teacher passes A and B against each other, accumulated into `counters` on the
    device.  cams / auxs: (A, B) pairs of min-max normalised CAMs [B,C,S,S]; tgts: the (A, B) cam-loss targets [B,C,h,w] or None; labels:
    the (A, B) main label maps [B,S,S]; aux_labels: the auxiliary pair or None; cls_label [B,C], or None: every plane is active.  Per
    map set the active planes' figure max |a - b| against `bar`, its histogram and worst value, the non-finite elements; per label pair
    agreement and per-class counts / intersections inside the boxes.  Every counter is an integer.  No host sync."""
    f = lambda t: t.detach().contiguous().float() if t is not None else None
    pair = lambda p: tuple(f(t) for t in p) if p is not None else None
    cams, auxs, tgts, labels, aux_labels, cls_label = pair(cams), pair(auxs), pair(tgts), pair(labels), pair(aux_labels), f(cls_label)
    _C.require_cuda(*cams, *auxs, *(tgts or ()), *labels, *(aux_labels or ()), cls_label, counters)
    B, C, K, S, h, w = _teacher_check_shapes(cams, auxs, tgts, labels, aux_labels, cls_label, counters)
    dev = cams[0].device
    boxes = _boxes_to_device(img_box, dev)
    if boxes.shape != (B, 4):
        raise ValueError("teacher_check: img_box must be [B,4]")
    L = _C.lib()
    ws = _C.workspace(L.cosa_teacher_check_workspace_bytes(B, C), dev, "teacher_check")
    none = (None, None)
    _C.check(L.cosa_teacher_check(*[_C.ptr(t) for t in cams + auxs + (tgts or none) + labels + (aux_labels or none)], _C.ptr(cls_label),
                                  _C.ptr(boxes), B, C, K, S, h, w, int(ignore_index), float(bar), _C.ptr(counters), _C.ptr(ws), ws.numel(),
                                  _C.stream_ptr()), "cosa_teacher_check")
    return counters


@torch.no_grad()
def teacher_check_torch(cams, auxs, tgts, labels, aux_labels, cls_label, img_box, counters, ignore_index=255, bar=TEACHER_CHECK_BAR):
    """teacher_check in plain torch, for host trainers and as the kernel's partner in the tests (the role label_stats_torch plays): the
    same counters in the same layout"""
    f = lambda t: t.detach().float() if t is not None else None
    pair = lambda p: tuple(f(t) for t in p) if p is not None else None
    cams, auxs, tgts, labels, aux_labels, cls_label = pair(cams), pair(auxs), pair(tgts), pair(labels), pair(aux_labels), f(cls_label)
    B, C, K, S, h, w = _teacher_check_shapes(cams, auxs, tgts, labels, aux_labels, cls_label, counters)
    if 0 <= int(ignore_index) < K or not float(bar) >= 0:
        raise ValueError("teacher_check: ignore_index must be no class and the bar a non-negative number")
    dev = cams[0].device
    off, _ = teacher_check_layout(K)
    add = torch.zeros_like(counters)
    add[off["checks"]] = 1
    active = (cls_label != 0) if cls_label is not None else torch.ones((B, C), dtype=torch.bool, device=dev)
    edges = torch.tensor(TEACHER_CHECK_EDGES, dtype=torch.float32, device=dev)
    bar32 = torch.tensor(float(bar), dtype=torch.float32, device=dev)
    worst = {}
    for name, ab in zip(TEACHER_CHECK_SETS, (cams, auxs, tgts)):
        if ab is None:
            continue
        a, b = ab
        bad_a, bad_b = ~torch.isfinite(a), ~torch.isfinite(b)
        d = torch.where(bad_a | bad_b, torch.full_like(a, float("inf")), (a - b).abs())          # (finite a - b: finite or inf, never NaN)
        fig = d.flatten(2).amax(dim=2)[active]                                                   # the active planes' figures, fp32
        add[off[name + ".planes"]] = fig.numel()
        add[off[name + ".over"]] = (fig > bar32).sum()
        add[off[name + ".hist"]:off[name + ".hist"] + len(TEACHER_CHECK_EDGES)] = \
            torch.bincount(torch.bucketize(fig, edges), minlength=len(TEACHER_CHECK_EDGES))        # first bin with fig <= edge
        add[off[name + ".nonfinite_a"]] = (bad_a & active[:, :, None, None]).sum()
        add[off[name + ".nonfinite_b"]] = (bad_b & active[:, :, None, None]).sum()
        worst[name] = fig.contiguous().view(torch.int32).max().long() if fig.numel() else torch.zeros((), dtype=torch.int64, device=dev)
    box = torch.as_tensor(img_box).to(device=dev, dtype=torch.int64)
    ar = torch.arange(S, device=dev)
    inside = ((ar[None, :, None] >= box[:, 0, None, None]) & (ar[None, :, None] < box[:, 1, None, None]) &
              (ar[None, None, :] >= box[:, 2, None, None]) & (ar[None, None, :] < box[:, 3, None, None]))
    for name, ab in zip(TEACHER_CHECK_PAIRS, (labels, aux_labels)):
        if ab is None:
            continue
        a, b = ab
        is_cls = lambda m: inside & (m >= 0) & (m < K) & (m == m.floor())                         # a value that is no label is counted nowhere
        add[off[name + ".pix"]] = inside.sum()
        add[off[name + ".agree"]] = (inside & (a == b)).sum()
        add[off[name + ".ign_a"]] = (inside & (a == ignore_index)).sum()
        add[off[name + ".ign_b"]] = (inside & (b == ignore_index)).sum()
        add[off[name + ".cnt_a"]:off[name + ".cnt_a"] + K] = torch.bincount(a[is_cls(a)].long(), minlength=K)
        add[off[name + ".cnt_b"]:off[name + ".cnt_b"] + K] = torch.bincount(b[is_cls(b)].long(), minlength=K)
        add[off[name + ".inter"]:off[name + ".inter"] + K] = torch.bincount(a[is_cls(a) & (a == b)].long(), minlength=K)
    counters += add
    for name, v in worst.items():                  # a maximum, not a sum: fp32 bit patterns of non-negative values order as integers
        o = off[name + ".worst"]
        counters[o] = torch.maximum(counters[o], v)
    return counters


def teacher_check_summary(counters, K):
    """The counter vector (tensor, array or list; a device tensor synchronises) as figures: per map set `worst` (a float), `over`,
    `planes`, `hist`, `nonfinite_a` / `nonfinite_b`; per label pair `agree` = agree / pix and `miou`, the mean of inter / (cnt_a + cnt_b -
    inter) over the classes with a non-zero union (`iou` the per-class list, None for an empty union); `checks`; and `conforms`: every over
    == 0, every agree >= 0.999 and every miou >= 0.999 over the sets and pairs that were counted -- the LITERAL leg of the criterion of
    tests/test_precision_gpu.py.  Its float64-bounded exemption for planes of conditioning > 50 is not evaluated (`exemption_evaluated`
    is False, `criterion` says so): a plane that the full criterion would exempt counts as over here.  `conforms_without_tgt` is the same
    verdict without the `tgt` set: the record's criterion speaks of the normalised CAMs and the masks only, and the cam-loss targets, a
    softmax at temperature --seg_softmaxtemp, magnify a logit difference up to 0.25 / T-fold where two classes tie.  Zero
    pixels or zero checks give agree = miou = 1.0 for an absent pair and both verdicts None when nothing was checked."""
    import struct
    c = [int(v) for v in (counters.tolist() if hasattr(counters, "tolist") else counters)]
    off, n = teacher_check_layout(K)
    if len(c) != n:
        raise ValueError(f"teacher_check_summary: {len(c)} counters, K = {K} has {n}")
    nb = len(TEACHER_CHECK_EDGES)
    out = {"checks": c[off["checks"]], "bar": TEACHER_CHECK_BAR, "hist_edges": [float(np.float32(e)) for e in TEACHER_CHECK_EDGES[:-1]] + ["inf"],
           "criterion": "literal bar only: max |a - b| per active plane <= bar, label agreement >= 0.999, mask mIoU >= 0.999; the "
                        "float64-bounded exemption for planes of conditioning > 50 is NOT evaluated",
           "exemption_evaluated": False}
    ok = ok_cams = True
    for s in TEACHER_CHECK_SETS:
        bits = c[off[s + ".worst"]]
        worst = struct.unpack("<f", struct.pack("<I", bits & 0xffffffff))[0]
        out[s] = {"planes": c[off[s + ".planes"]], "over": c[off[s + ".over"]], "worst": worst if math.isfinite(worst) else "inf",
                  "worst_bits": bits, "hist": c[off[s + ".hist"]:off[s + ".hist"] + nb],
                  "nonfinite_a": c[off[s + ".nonfinite_a"]], "nonfinite_b": c[off[s + ".nonfinite_b"]]}
        ok = ok and out[s]["over"] == 0
        ok_cams = ok_cams and (s == "tgt" or out[s]["over"] == 0)
    for p in TEACHER_CHECK_PAIRS:
        pix = c[off[p + ".pix"]]
        ca, cb, it = (c[off[f"{p}.{f}"]:off[f"{p}.{f}"] + K] for f in ("cnt_a", "cnt_b", "inter"))
        union = [a + b - i for a, b, i in zip(ca, cb, it)]
        iou = [i / u if u else None for i, u in zip(it, union)]
        live = [v for v in iou if v is not None]
        out[p] = {"pix": pix, "agree": c[off[p + ".agree"]] / pix if pix else 1.0, "miou": sum(live) / len(live) if live else 1.0,
                  "iou": iou, "ign_a": c[off[p + ".ign_a"]], "ign_b": c[off[p + ".ign_b"]]}
        pair_ok = out[p]["agree"] >= TEACHER_CHECK_AGREE and out[p]["miou"] >= TEACHER_CHECK_MIOU
        ok, ok_cams = ok and pair_ok, ok_cams and pair_ok
    out["conforms"] = bool(ok) if out["checks"] else None
    out["conforms_without_tgt"] = bool(ok_cams) if out["checks"] else None
    return out


def teacher_check_worst(summary):
    """the figures of a summary that a log line shows: the worst over the map sets and over the label pairs that were counted"""
    sets = [summary[s] for s in TEACHER_CHECK_SETS if summary[s]["planes"]]
    pairs = [summary[p] for p in TEACHER_CHECK_PAIRS if summary[p]["pix"]]
    worst = max([float(s["worst"]) for s in sets], default=0.0)
    return {"worst": worst, "over": sum(s["over"] for s in sets), "planes": sum(s["planes"] for s in sets),
            "agree": min([p["agree"] for p in pairs], default=1.0), "miou": min([p["miou"] for p in pairs], default=1.0)}


# --------------------------------------------------------------------------------------------
# the conformance criterion per plane on the device (DESIGN.md sections 3 and 20): rules (a) literal bar and (b) float64-bounded exemption
# --------------------------------------------------------------------------------------------
CAM_BAR, COND_MAX, FP64_FACTOR = 1e-3, 50.0, 4.0                  # THE product's copy of the pre-registered constants (tests/test_precision_gpu.py)
AGREE_BAR, MIOU_BAR = 0.999, 0.999                                # rule (c): label agreement per draw, pooled mask mIoU
CONFORMANCE_FIGS = ("d", "lit", "cond", "own", "e_ref", "e_hip", "bound", "max32")      # the columns of cosa_conformance_planes
assert len(CONFORMANCE_FIGS) == _C.constant("COSA_CONFORMANCE_FIGS")
CONFORMANCE_VERDICTS = {-1: "inactive", 0: "ok", 1: "exempt", 2: "fail"}


def conformance_planes(camA, cam32, cam64, active, peak64, rawmax64, cam_bar=CAM_BAR, cond_max=COND_MAX, fp64_factor=FP64_FACTOR):
    """The criterion's rules (a) and (b) for every plane of one CAM set, by one launch (cosa_conformance_planes): camA [B,C,S,S] fp32 the mode
    under test, cam32 the "fp32" pass, cam64 float64, active [B,C] (or None: every plane), peak64 / rawmax64 [B,C] float64 from the float64
    pass (multi_scale_camseg(..., _return_scale=True)).  -> {"fig": [B,C,8] float64 in CONFORMANCE_FIGS order, "verdict": [B,C] int32 (-1
    inactive, 0 ok, 1 exempt, 2 fail), "nonfinite": [B,C] int32}.  A float64 camA / cam32 is rounded to fp32 here, once.  No host sync."""
    f32 = lambda t: t.detach().contiguous().float()
    camA, cam32 = f32(camA), f32(cam32)
    cam64, peak64, rawmax64 = (t.detach().contiguous() for t in (cam64, peak64, rawmax64))
    act = f32(active) if active is not None else None
    _C.require_cuda(camA, cam32, cam64, act, peak64, rawmax64)
    B, C, S, S2 = camA.shape
    if cam32.shape != camA.shape or cam64.shape != camA.shape or cam64.dtype != torch.float64 or peak64.shape != (B, C) or rawmax64.shape != (B, C) \
            or peak64.dtype != torch.float64 or rawmax64.dtype != torch.float64 or (act is not None and act.shape != (B, C)):
        raise ValueError("conformance_planes: the three CAM sets must be [B,C,S,S] (cam64 float64), active / peak64 / rawmax64 [B,C] (the last two float64)")
    fig = torch.empty((B, C, len(CONFORMANCE_FIGS)), device=camA.device, dtype=torch.float64)
    vd = torch.empty((B, C, 2), device=camA.device, dtype=torch.int32)
    _C.check(_C.lib().cosa_conformance_planes(_C.ptr(camA), _C.ptr(cam32), _C.ptr(cam64), _C.ptr(act), _C.ptr(peak64), _C.ptr(rawmax64), B * C, S * S2,
                                              float(cam_bar), float(cond_max), float(fp64_factor), _C.ptr(fig), _C.ptr(vd), _C.stream_ptr()),
             "cosa_conformance_planes")
    return {"fig": fig, "verdict": vd[:, :, 0], "nonfinite": vd[:, :, 1]}


def conformance_summary(tables):
    """{set name: conformance_planes table} (tensors or arrays; device tensors synchronise) -> per set planes / literal_ok / exempt / failed,
    the worst lit / own / cond / e_hip over the active planes, and `over`: one record per plane over the literal bar (img, cls, cond, lit, own,
    e_hip, bound, verdict)"""
    out = {}
    for name, t in tables.items():
        fig, vd = (np.asarray(t[k].cpu() if hasattr(t[k], "cpu") else t[k]) for k in ("fig", "verdict"))
        live = vd >= 0
        col = lambda k: fig[:, :, CONFORMANCE_FIGS.index(k)]
        worst = {k: (float(col(k)[live].max()) if live.any() else 0.0) for k in ("lit", "own", "cond", "e_hip")}
        over = [{"img": int(i), "cls": int(c), "verdict": CONFORMANCE_VERDICTS[int(vd[i, c])],
                 **{k: float(col(k)[i, c]) for k in ("cond", "lit", "own", "e_hip", "bound")}} for i, c in zip(*np.nonzero(vd > 0))]
        out[name] = {"planes": int(live.sum()), "literal_ok": int((vd == 0).sum()), "exempt": int((vd == 1).sum()), "failed": int((vd == 2).sum()),
                     "worst": worst, "over": over}
    return out


def conformance_line(s):
    """one set of a conformance_summary in the accuracy record's format (tests/test_precision_gpu.py: `| planes N literal-ok L ...`)"""
    notes = [f"[img {r['img']} cls {r['cls']}: cond {r['cond']:.1f} lit {r['lit']:.3e} own {r['own']:.3e} fp64 {r['e_hip']:.3e} bound {r['bound']:.3e} "
             f"{'ok' if r['verdict'] == 'exempt' else 'FAIL'}]" for r in s["over"]]
    return " ".join([f"planes {s['planes']} literal-ok {s['literal_ok']} exempt {s['exempt']} fail {s['failed']}"] + notes)


# --------------------------------------------------------------------------------------------
# the --student_check monitor: the student's training forward against a second forward of the same weights
# --------------------------------------------------------------------------------------------
STUDENT_CHECK_TENSORS = ("seg", "cam", "cam_aux", "cls", "cls_aux")            # include/cosa_hip.h: the counter vector's order
_SC_FIELDS = ("n", "nonfinite_a", "nonfinite_b", "max_abs", "range", "sum_d2", "sum_b2")
STUDENT_CHECK_LOSSES = ("cls_loss", "cls_loss_aux", "seg_loss", "cam_loss")
_SC_LOSS_FIELDS = ("sum_d", "sum_b", "max_abs", "n")
STUDENT_CHECK_EDGES = (1e-3, 1e-2, 1e-1)                                        # upper edges (fp32, exclusive) of the flip histogram's first three bins
STUDENT_CHECK_HEAD, STUDENT_CHECK_MAX_K = _C.constant("COSA_STUDENT_CHECK_HEAD"), _C.constant("COSA_STUDENT_CHECK_MAX_K")
STUDENT_CHECK_FIXED = {k: (_C.constant(f"COSA_STUDENT_CHECK_{k.upper()}_FRAC"), _C.constant(f"COSA_STUDENT_CHECK_{k.upper()}_INT"))
                       for k in ("d2", "b2", "loss")}                           # (fractional bits, a term must be < 2^int)


def student_check_layout(K):
    """({slot name: offset in elements}, number of elements) of cosa_student_check's counter vector for K = num_classes (background
    included): "checks", "flags", "<tensor>.<field>" for seg / cam / cam_aux / cls / cls_aux, "cells", "differ", "flip_hist" (4 bins),
    "cls.sign_flips", "cls_aux.sign_flips", "cls_cols", "<loss>.<field>", "labelled" (K) and "agree" (K).  Needs no device."""
    n = _C.lib().cosa_student_check_counters(int(K))
    if n == 0:
        raise ValueError(_C.lib().cosa_last_error().decode("utf-8", "replace"))
    off = {"checks": 0, "flags": 1}
    for t, name in enumerate(STUDENT_CHECK_TENSORS):
        for f, field in enumerate(_SC_FIELDS):
            off[f"{name}.{field}"] = 2 + len(_SC_FIELDS) * t + f
    off.update({"cells": 37, "differ": 38, "flip_hist": 39, "cls.sign_flips": 43, "cls_aux.sign_flips": 44, "cls_cols": 45})
    for j, name in enumerate(STUDENT_CHECK_LOSSES):
        for f, field in enumerate(_SC_LOSS_FIELDS):
            off[f"{name}.{field}"] = 46 + len(_SC_LOSS_FIELDS) * j + f
    off["labelled"], off["agree"] = STUDENT_CHECK_HEAD, STUDENT_CHECK_HEAD + int(K)
    assert int(n) == STUDENT_CHECK_HEAD + 2 * int(K)
    return off, int(n)


def new_student_check(K, device):
    """a zeroed counter vector (int64: the uint64 counters of the C ABI, which stay below 2^63)"""
    return _new_counters(student_check_layout(K), device)


def _student_check_shapes(seg, cam, aux, cls, clsaux, losses, cls_label, counters):
    B, K = seg[0].shape[:2]
    h, w = (int(v) for v in seg[0].shape[-2:])
    ok = seg[0].dim() == 4 and all(t.shape == (B, K, h, w) for t in seg) and all(t.shape == (B, K - 1, h, w) for t in tuple(cam) + tuple(aux)) and \
        all(t.shape == (B, K - 1) for t in tuple(cls) + tuple(clsaux) + (cls_label,)) and all(t.shape == (4,) for t in losses)
    if not ok:
        raise ValueError("student_check: the seg pair must be [B,K,h,w], the CAM pairs [B,K-1,h,w], the cls pairs and cls_label [B,K-1] and "
                         "the loss vectors [4]")
    if K < 2 or K > STUDENT_CHECK_MAX_K or B * K * h * w >= 2 ** 31:
        raise ValueError(f"student_check: outside the envelope (2 <= K {K} <= {STUDENT_CHECK_MAX_K}, B K h w < 2^31)")
    _check_counters(counters, student_check_layout(K), "student_check")
    return int(B), int(K), h, w


def student_check(seg, cam, aux, cls, clsaux, losses, cls_label, counters):
    """One reduction (cosa_student_check) that scores two forwards of the student against each other, accumulated into `counters` on the
    device.  Every argument but the last two is an (a, b) pair, a the training forward, b the check pass: seg logits [B,K,h,w], CAMs and
    auxiliary CAMs [B,K-1,h,w], classification logits and auxiliary ones [B,K-1], loss vectors [4] (cls_loss, cls_loss_aux, seg_loss,
    cam_loss); cls_label [B,K-1].  Per tensor, over the background and the present classes: elements, non-finite counts, max |a - b|,
    max |b|, sum (a - b)^2 and sum b^2 in fixed point; the seg decisions per cell; the classification sign flips; the loss terms.  Every
    counter is an integer.  No host sync."""
    f = lambda t: t.detach().contiguous().float()
    seg, cam, aux, cls, clsaux, losses = (tuple(f(t) for t in p) for p in (seg, cam, aux, cls, clsaux, losses))
    cls_label = f(cls_label)
    _C.require_cuda(*seg, *cam, *aux, *cls, *clsaux, *losses, cls_label, counters)
    B, K, h, w = _student_check_shapes(seg, cam, aux, cls, clsaux, losses, cls_label, counters)
    _C.check(_C.lib().cosa_student_check(*[_C.ptr(t) for t in seg + cam + aux + cls + clsaux + losses], _C.ptr(cls_label), _C.ptr(counters),
                                         B, K, h, w, _C.stream_ptr()), "cosa_student_check")
    return counters


def _sc_fixed(term, kind):
    """fp32 terms -> (int64 fixed-point values, mask of the representable ones): rint(term * 2^frac) in double where term < 2^int"""
    frac, bits = STUDENT_CHECK_FIXED[kind]
    ok = term < float(2 ** bits)                                                   # (False for NaN and +inf)
    v = torch.where(ok, term, torch.zeros_like(term)).double() * float(2 ** frac)
    return torch.round(v).long(), ok                                               # (torch.round: half to even, like rint)


@torch.no_grad()
def student_check_torch(seg, cam, aux, cls, clsaux, losses, cls_label, counters):
    """student_check in plain torch, for host trainers and as the kernel's partner in the tests: the same counters in the same layout"""
    f = lambda t: t.detach().float()
    seg, cam, aux, cls, clsaux, losses = (tuple(f(t) for t in p) for p in (seg, cam, aux, cls, clsaux, losses))
    cls_label = f(cls_label)
    B, K, h, w = _student_check_shapes(seg, cam, aux, cls, clsaux, losses, cls_label, counters)
    dev = seg[0].device
    off, n = student_check_layout(K)
    add = torch.zeros(n, dtype=torch.int64, device=dev)
    mx = torch.zeros(n, dtype=torch.int64, device=dev)
    flags = torch.zeros((), dtype=torch.int64, device=dev)
    bits = lambda v: v.contiguous().view(torch.int32).long()                       # of non-negative fp32 values
    present = cls_label != 0
    allowed = torch.cat([torch.ones(B, 1, dtype=torch.bool, device=dev), present], dim=1)          # seg channels: background + present classes
    masks = (allowed[:, :, None, None].expand(B, K, h, w), present[:, :, None, None].expand(B, K - 1, h, w),
             present[:, :, None, None].expand(B, K - 1, h, w), present, present)
    for t, (name, (a, b), m) in enumerate(zip(STUDENT_CHECK_TENSORS, (seg, cam, aux, cls, clsaux), masks)):
        a, b = a[m], b[m]
        fa, fb = torch.isfinite(a), torch.isfinite(b)
        both = fa & fb
        add[off[name + ".n"]] = a.numel()
        add[off[name + ".nonfinite_a"]] = (~fa).sum()
        add[off[name + ".nonfinite_b"]] = (~fb).sum()
        d = (a[both] - b[both])
        bb = b[both]
        dfin = d[torch.isfinite(d)].abs()
        if dfin.numel():
            mx[off[name + ".max_abs"]] = bits(dfin).max()
        if fb.any():
            mx[off[name + ".range"]] = bits(b[fb].abs()).max()
        v1, ok1 = _sc_fixed(d * d, "d2")
        v2, ok2 = _sc_fixed(bb * bb, "b2")
        add[off[name + ".sum_d2"]] = v1.sum()
        add[off[name + ".sum_b2"]] = v2.sum()
        bad = (~both).any() | (~ok1).any() | (~ok2).any()
        flags = flags | (bad.long() << t)
    # the seg decisions: argmax over the allowed channels, NaN read as -inf, the lowest channel among equals
    ninf = torch.full((), float("-inf"), device=dev)
    ch = torch.arange(K, device=dev)[None, :, None, None]
    am = allowed[:, :, None, None]

    def decide(x):
        v = torch.where(am & ~torch.isnan(x), x, ninf)
        top = v.amax(dim=1, keepdim=True)
        idx = torch.where((v == top) & am, ch, torch.full_like(ch, K)).amin(dim=1, keepdim=True)
        second = torch.where(am & (ch != idx), v, ninf).amax(dim=1)
        return idx[:, 0], top[:, 0], second

    ia, _, _ = decide(seg[0])
    ib, top_b, second_b = decide(seg[1])
    differ = ia != ib
    add[off["cells"]] = ia.numel()
    add[off["differ"]] = differ.sum()
    margin = (top_b - second_b)[differ]
    e = [torch.tensor(v, dtype=torch.float32, device=dev) for v in STUDENT_CHECK_EDGES]
    bins = 3 - ((margin < e[0]).long() + (margin < e[1]).long() + (margin < e[2]).long())         # (a NaN margin: the last bin)
    add[off["flip_hist"]:off["flip_hist"] + 4] = torch.bincount(bins.reshape(-1), minlength=4)
    add[off["labelled"]:off["labelled"] + K] = torch.bincount(ib.reshape(-1), minlength=K)
    add[off["agree"]:off["agree"] + K] = torch.bincount(ib[~differ].reshape(-1), minlength=K)
    for name, (a, b) in (("cls", cls), ("cls_aux", clsaux)):
        add[off[name + ".sign_flips"]] = (torch.sign(torch.nan_to_num(a, nan=0.0)) != torch.sign(torch.nan_to_num(b, nan=0.0))).sum()
    add[off["cls_cols"]] = B * (K - 1)
    la, lb = losses
    for j, name in enumerate(STUDENT_CHECK_LOSSES):
        a, b = la[j], lb[j]
        d = (a - b).abs()
        v1, ok1 = _sc_fixed(d.reshape(1), "loss")
        v2, ok2 = _sc_fixed(b.abs().reshape(1), "loss")
        good = torch.isfinite(a) & torch.isfinite(b) & ok1[0] & ok2[0]
        add[off[name + ".sum_d"]] = torch.where(good, v1[0], torch.zeros_like(v1[0]))
        add[off[name + ".sum_b"]] = torch.where(good, v2[0], torch.zeros_like(v2[0]))
        mx[off[name + ".max_abs"]] = torch.where(good, bits(torch.where(good, d, torch.zeros_like(d)).reshape(1))[0], torch.zeros((), dtype=torch.int64, device=dev))
        add[off[name + ".n"]] = 1
        flags = flags | ((~good).long() << (8 + j))
    add[off["checks"]] = 1
    counters += add
    torch.maximum(counters, mx, out=counters)            # (a slot that holds a maximum is never added to, and the other slots only grow)
    counters[off["flags"]] |= flags
    return counters


def student_check_summary(counters, K):
    """The counter vector (tensor, array or list; a device tensor synchronises) as figures: per tensor `rel_l2` = sqrt(sum (a - b)^2 / sum b^2),
    `max_abs`, `range` (the largest |b|), `n` and the non-finite counts; `seg_agree`, the share of cells with the same argmax; `flip_hist`,
    the differing cells by the check pass's margin (`flip_edges`); `class_agree`, per class agree / labelled (None for a class the check
    pass labels nowhere); `cls_sign_flips` and `cls_aux_sign_flips`; per loss term `loss_rel` = sum |a - b| / sum |b| and `max_abs`;
    `checks` and `flags` (0: every term was representable).  Empty sums give 0.0, zero cells seg_agree = 1.0."""
    import struct
    c = [int(v) for v in (counters.tolist() if hasattr(counters, "tolist") else counters)]
    off, n = student_check_layout(K)
    if len(c) != n:
        raise ValueError(f"student_check_summary: {len(c)} counters, K = {K} has {n}")
    as_f = lambda b: struct.unpack("<f", struct.pack("<I", b & 0xffffffff))[0]
    fx = STUDENT_CHECK_FIXED
    out = {"checks": c[off["checks"]], "flags": c[off["flags"]], "flip_edges": [float(np.float32(e)) for e in STUDENT_CHECK_EDGES]}
    for t in STUDENT_CHECK_TENSORS:
        sd2, sb2 = c[off[t + ".sum_d2"]] / 2.0 ** fx["d2"][0], c[off[t + ".sum_b2"]] / 2.0 ** fx["b2"][0]
        out[t] = {"n": c[off[t + ".n"]], "rel_l2": math.sqrt(sd2 / sb2) if sb2 > 0 else 0.0, "max_abs": as_f(c[off[t + ".max_abs"]]),
                  "range": as_f(c[off[t + ".range"]]), "nonfinite_a": c[off[t + ".nonfinite_a"]], "nonfinite_b": c[off[t + ".nonfinite_b"]]}
    cells, differ = c[off["cells"]], c[off["differ"]]
    out["cells"] = cells
    out["seg_agree"] = (cells - differ) / cells if cells else 1.0
    out["flip_hist"] = c[off["flip_hist"]:off["flip_hist"] + 4]
    lab, agr = c[off["labelled"]:off["labelled"] + K], c[off["agree"]:off["agree"] + K]
    out["class_agree"] = [a / l if l else None for a, l in zip(agr, lab)]
    out["class_cells"] = lab
    out["cls_sign_flips"], out["cls_aux_sign_flips"], out["cls_cols"] = c[off["cls.sign_flips"]], c[off["cls_aux.sign_flips"]], c[off["cls_cols"]]
    out["losses"] = {}
    for l in STUDENT_CHECK_LOSSES:
        sd, sb = c[off[l + ".sum_d"]] / 2.0 ** fx["loss"][0], c[off[l + ".sum_b"]] / 2.0 ** fx["loss"][0]
        out["losses"][l] = {"loss_rel": sd / sb if sb > 0 else 0.0, "max_abs": as_f(c[off[l + ".max_abs"]]), "n": c[off[l + ".n"]]}
    live = [v["loss_rel"] for v in out["losses"].values()]
    out["loss_rel"] = max(live) if live else 0.0
    return out


# --------------------------------------------------------------------------------------------
# the --act_stats_iters monitor: activation range and attention sharpness of an fp32 pass on the teacher's weights
# --------------------------------------------------------------------------------------------
ACT_STATS_SITES = ("q", "k", "v", "o", "h", "x")                               # models/vit.py: ACT_SITES, the order of a block's range sites
ACT_STATS_F16_SITES = ("q", "k", "v", "o", "h")                                 # ... those an fp16x3 pass stores as fp16 halves (x is the fp32 stream)
_AS_RANGE_FIELDS = ("finite", "absmax", "over", "near", "tiny", "nonfinite")    # cosa_range_stats_f32's six words
_AS_HEAD_FIELDS = ("rows", "ent_fix", "top1_fix", "peaked", "smax", "sharp", "nonfinite_rows")      # cosa_attn_stats_f32's seven per head
ACT_STATS_FRAC = _C.constant("COSA_ACT_STATS_FRAC")                             # ent_fix and top1_fix count 2^-32
F16_MAX = 65504.0


def act_stats_layout(depth, H):
    """({slot name: offset in elements}, number of elements) of the --act_stats counters for `depth` blocks of H heads: block i holds
    "<i>.<site>.<field>" for the sites q, k, v, o, h, x (six words each: finite, absmax, over, near, tiny, nonfinite) at i * W + 6 * site,
    then "<i>.head<h>.<field>" (seven each: rows, ent_fix, top1_fix, peaked, smax, sharp, nonfinite_rows) at i * W + 36 + 7 * h, with
    W = "width" = 36 + 7 H; "checks", the passes accumulated, is the last element (depth * W).  The first depth * W elements viewed as
    [depth][W] are the table an encoder's act_probe adds into.  Needs no device."""
    depth, H = int(depth), int(H)
    if depth < 1 or H < 1:
        raise ValueError(f"act_stats_layout: depth {depth} and heads {H} must be positive")
    W = len(_AS_RANGE_FIELDS) * len(ACT_STATS_SITES) + len(_AS_HEAD_FIELDS) * H
    off = {"width": W}
    for i in range(depth):
        for j, site in enumerate(ACT_STATS_SITES):
            for f, field in enumerate(_AS_RANGE_FIELDS):
                off[f"{i}.{site}.{field}"] = i * W + 6 * j + f
        for h in range(H):
            for f, field in enumerate(_AS_HEAD_FIELDS):
                off[f"{i}.head{h}.{field}"] = i * W + 36 + 7 * h + f
    off["checks"] = depth * W
    return off, depth * W + 1


def new_act_stats(depth, H, device):
    """a zeroed counter vector (int64) of act_stats_layout's length"""
    return _new_counters(act_stats_layout(depth, H), device)


def act_stats_table(counters, depth, H):
    """the [depth][36 + 7 H] view of a counter vector that an ActProbe takes as its table"""
    W = act_stats_layout(depth, H)[0]["width"]
    return counters[:int(depth) * W].view(int(depth), W)


def act_stats_summary(counters, depth, H):
    """The counter vector (tensor, array or list; a device tensor synchronises) as figures.  `layers`[i]: `sites` {site: absmax, over, near,
    tiny, nonfinite, finite} and `heads`[h] {rows, ent (mean normalised row entropy), top1 (mean largest probability), peaked (share of rows
    with top1 > 0.5), smax (largest |logit| after the scale), sharpest (the lowest row entropy seen: 1 - max(1 - Hn); None: no row),
    nonfinite_rows}.  Globals: `headroom_bits` = log2(65504 / absmax) at its minimum over the sites an fp16 split stores (q, k, v, o, h)
    with `headroom_at` [site, layer] (None while every such site is zero or unseen); `smax` with `smax_at` [layer, head]; `ent_mean` (over
    all rows) and `ent_min` with `ent_min_at` [layer, head]; `over` (those five sites) and `nonfinite` (all six, plus `nonfinite_rows`);
    `checks`."""
    import struct
    c = [int(v) for v in (counters.tolist() if hasattr(counters, "tolist") else counters)]
    off, n = act_stats_layout(depth, H)
    if len(c) != n:
        raise ValueError(f"act_stats_summary: {len(c)} counters, depth {depth} x {H} heads has {n}")
    as_f = lambda b: struct.unpack("<f", struct.pack("<I", b & 0xffffffff))[0]
    unit = 2.0 ** ACT_STATS_FRAC
    out = {"checks": c[off["checks"]], "layers": [], "headroom_bits": None, "headroom_at": None, "smax": 0.0, "smax_at": None,
           "ent_mean": None, "ent_min": None, "ent_min_at": None, "over": 0, "nonfinite": 0, "nonfinite_rows": 0}
    rows_all = ent_all = 0
    for i in range(depth):
        sites, heads = {}, []
        for site in ACT_STATS_SITES:
            g = lambda f: c[off[f"{i}.{site}.{f}"]]
            e = {"absmax": as_f(g("absmax")), "over": g("over"), "near": g("near"), "tiny": g("tiny"), "nonfinite": g("nonfinite"),
                 "finite": g("finite")}
            sites[site] = e
            out["nonfinite"] += e["nonfinite"]
            if site in ACT_STATS_F16_SITES:
                out["over"] += e["over"]
                if e["absmax"] > 0:
                    bits = math.log2(F16_MAX / e["absmax"])
                    if out["headroom_bits"] is None or bits < out["headroom_bits"]:
                        out["headroom_bits"], out["headroom_at"] = bits, [site, i]
        for h in range(H):
            g = lambda f: c[off[f"{i}.head{h}.{f}"]]
            rows = g("rows")
            e = {"rows": rows, "ent": g("ent_fix") / unit / rows if rows else None, "top1": g("top1_fix") / unit / rows if rows else None,
                 "peaked": g("peaked") / rows if rows else None, "smax": as_f(g("smax")),
                 "sharpest": 1.0 - as_f(g("sharp")) if rows else None, "nonfinite_rows": g("nonfinite_rows")}
            heads.append(e)
            out["nonfinite_rows"] += e["nonfinite_rows"]
            rows_all += rows
            ent_all += g("ent_fix")
            if rows and (out["smax_at"] is None or e["smax"] > out["smax"]):
                out["smax"], out["smax_at"] = e["smax"], [i, h]
            if rows and (out["ent_min"] is None or e["ent"] < out["ent_min"]):
                out["ent_min"], out["ent_min_at"] = e["ent"], [i, h]
        out["layers"].append({"sites": sites, "heads": heads})
    if rows_all:
        out["ent_mean"] = ent_all / unit / rows_all
    return out


def act_stats_line(s):
    """` act: headroom 9.3b (h L11), max|s| 41.2 (L9 h3), ent 0.62 (min 0.31 L9 h3), over 0` -- the bits left under 65504 at the site and
    block closest to it, the largest attention logit with its block and head, the mean normalised row entropy with the lowest head's, and
    the elements an fp16 half could not hold; `-` where nothing was seen"""
    head = "headroom %.1fb (%s L%d)" % (s["headroom_bits"], s["headroom_at"][0], s["headroom_at"][1]) if s["headroom_bits"] is not None else "headroom -"
    if s["smax_at"] is None:
        return " act: %s, max|s| -, ent -, over %d" % (head, s["over"])
    return " act: %s, max|s| %.1f (L%d h%d), ent %.2f (min %.2f L%d h%d), over %d" % (
        head, s["smax"], s["smax_at"][0], s["smax_at"][1], s["ent_mean"], s["ent_min"], s["ent_min_at"][0], s["ent_min_at"][1], s["over"])


def seg_loss_forward_only(seg_lr, mask_main, mask_aux, img, img_box, fg_alpha=0.5, aux_alpha=0.5, rel_main=None, rel_aux=None):
    """the seg-loss half of fused_seg_and_energy_loss by its forward kernel alone (_seg_loss_launch, _seg_loss_value: the same call, the
    same value): no regulariser, nothing kept for a backward.  For the --student_check pass.  rel_main / rel_aux: the step's weight maps
    (--seg_reliability), as fused_seg_and_energy_loss takes them."""
    boxes = _boxes_to_device(img_box, seg_lr.device)
    weights = seg_blend_weights(fg_alpha, aux_alpha, mask_aux is not None)
    rel = _rel_pair(rel_main, rel_aux, mask_aux)
    return _seg_loss_value(_seg_loss_launch(seg_lr.detach(), mask_main, mask_aux, img, boxes, weights, rel)[0], weights)


EXPORT_BITS = {k: _C.constant("COSA_EXPORT_" + k.upper()) for k in ("seg", "pseudo", "pseudo_aux", "rawcam", "rawcam_aux", "pseudo_par", "pseudo_aux_par")}
_EXPORT_SLOTS = ("seg", "pseudo", "pseudo_aux", "rawcam", "rawcam_aux", "rawcam_idx", "rawcam_aux_idx", "pseudo_par", "pseudo_aux_par")
assert len(_EXPORT_SLOTS) == _C.constant("COSA_EXPORT_SLOTS")
EXPORT_MAPS_MASK = _C.constant("COSA_EXPORT_ALL")                               # the products cosa_export_maps writes; cosa_export_refine writes the PAR ones
EXPORT_PAR_MASK = EXPORT_BITS["pseudo_par"] | EXPORT_BITS["pseudo_aux_par"]
EXPORT_REFINE_MIN_SIDE = _C.constant("COSA_EXPORT_REFINE_MIN_SIDE")
PAR_DILATIONS, PAR_NUM_ITER = (1, 2, 4, 8, 12, 24), 10   # the refine model CoSA trains with (main.py: PAR(num_iter=10, dilations=[1,2,4,8,12,24]))


def export_what_mask(what):
    """("seg", "pseudo", ...) or a ready bit mask -> the COSA_EXPORT_* mask; unknown names are an error"""
    if isinstance(what, int):
        return what
    unknown = [w for w in what if w not in EXPORT_BITS]
    if unknown or not len(what):
        raise ValueError(f"export products must be some of {sorted(EXPORT_BITS)}, got {list(what)}")
    m = 0
    for w in what:
        m |= EXPORT_BITS[w]
    return m


def export_record_layout(C, H, W, k_live, what):
    """cosa_export_record_layout: ({slot name: byte offset} of the products asked for, record size in bytes).  Needs no device."""
    off = (ctypes.c_size_t * len(_EXPORT_SLOTS))()
    n = _C.lib().cosa_export_record_layout(int(C), int(H), int(W), int(k_live), export_what_mask(what), off)
    if n == 0:
        _C.check(1, "cosa_export_record_layout")
    none = ctypes.c_size_t(-1).value
    return {k: int(o) for k, o in zip(_EXPORT_SLOTS, off) if o != none}, int(n)


def export_record_views(record, C, H, W, k_live, what):
    """the products inside a packed record (a uint8 tensor on any device, or a numpy uint8 array), as views: uint8 [H,W] maps,
    rawcam* float32 [k_live,H,W] and rawcam*_idx int32 [k_live]"""
    offs, _ = export_record_layout(C, H, W, k_live, what)
    out = {}
    for k, o in offs.items():
        if k in ("rawcam", "rawcam_aux"):
            out[k] = record[o:o + 4 * k_live * H * W].view(torch.float32 if torch.is_tensor(record) else np.float32).reshape(k_live, H, W)
        elif k.endswith("_idx"):
            out[k] = record[o:o + 4 * k_live].view(torch.int32 if torch.is_tensor(record) else np.int32)
        else:
            out[k] = record[o:o + H * W].reshape(H, W)
    return out


def export_maps(cam, cam_aux, seg, cls_label, size, what, high_thre, low_thre, ignore_index=255, out=None, k_live=None):
    """Every file product of ONE image in one launch and one packed record (cosa_export_maps).
    cam / cam_aux [1,C,S,S] or [C,S,S], seg [1,C+1,S,S] or [C+1,S,S] as multi_scale_camsegv3 returns them, cls_label [1,C] / [C] or
    None (no image-level labels: "seg" only, the plain argmax).  `what`: names out of seg, pseudo, pseudo_aux, rawcam, rawcam_aux.
    `out`: a caller-owned uint8 device record to write into (at least the layout's size); `k_live`: the number of present classes when the
    caller knows it on the host -- without it the label row is counted here, which waits for the device.
    Returns views into the record (export_record_views): uint8 [H,W] maps, rawcam* float32 [k_live,H,W], rawcam*_idx int32 [k_live].
    The PAR-refined products are export_refine's, not this function's."""
    H, W = int(size[0]), int(size[1])
    mask = export_what_mask(what)
    if mask & EXPORT_PAR_MASK:
        raise ValueError("export_maps: pseudo_par / pseudo_aux_par are written by export_refine")
    ref = seg if seg is not None else (cam if cam is not None else cam_aux)
    if ref is None:
        raise ValueError("export_maps: no input maps")
    _C.require_cuda(cam, cam_aux, seg, cls_label, out)
    S = ref.shape[-1]
    prep = lambda t: t.contiguous().float() if t is not None else None
    cam, cam_aux, seg, cls = prep(cam), prep(cam_aux), prep(seg), prep(cls_label)
    if cls is not None:
        C = cls.numel()
    else:
        C = seg.shape[-3] - 1 if seg is not None else ref.shape[-3]
    for t, ch, nm in ((cam, C, "cam"), (cam_aux, C, "cam_aux"), (seg, C + 1, "seg")):
        if t is not None and (t.numel() != ch * S * S or tuple(t.shape[-3:]) != (ch, S, S)):
            raise ValueError(f"export_maps: {nm} must be one image's [{ch},{S},{S}], got {tuple(t.shape)}")
    if k_live is None:
        k_live = int((cls != 0).sum()) if cls is not None else 0
    offs, nbytes = export_record_layout(C, H, W, k_live, mask)
    if out is None:
        out = torch.empty(nbytes, device=ref.device, dtype=torch.uint8)
    elif out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() < nbytes:
        raise ValueError(f"export_maps: `out` must be a contiguous uint8 record of at least {nbytes} bytes")
    _C.check(_C.lib().cosa_export_maps(_C.ptr(cam), _C.ptr(cam_aux), _C.ptr(seg), _C.ptr(cls), C, S, H, W, int(k_live), mask,
                                       float(high_thre if high_thre is not None else 0.0), float(low_thre if low_thre is not None else 0.0),
                                       int(ignore_index), _C.ptr(out), out.numel(), _C.stream_ptr()), "cosa_export_maps")
    return export_record_views(out, C, H, W, k_live, mask)


def export_refine(image, cam, cam_aux, cls_label, what, high_thre, low_thre, ignore_index=255, downscale=2, dilations=PAR_DILATIONS,
                  num_iter=PAR_NUM_ITER, out=None, k_live=None):
    """The PAR-refined pseudo labels of ONE image at its own size (cosa_export_refine): the reference's
    `cam2mask(image, [[0,H,0,W]], cls * resize(cam, (H,W)), cls, high, low, refine_model=PAR(num_iter, dilations), downscale)` for the
    main and / or the auxiliary CAMs in one pass -- one affinity tensor, one stream of it per propagation step.
    image [1,3,H,W] / [3,H,W] in [0,1] (torch_helper.denormalize_img), cam / cam_aux [1,C,S,S] or [C,S,S], cls_label [1,C] / [C].
    `what`: the products of the record (`out`, as export_maps lays it out), at least one of pseudo_par, pseudo_aux_par; only those two
    slots are written.  downscale 2 or 0; H, W >= EXPORT_REFINE_MIN_SIDE.  Returns {product: uint8 [H,W] view} of the PAR products."""
    mask = export_what_mask(what)
    if not mask & EXPORT_PAR_MASK:
        raise ValueError(f"export_refine: `what` names neither pseudo_par nor pseudo_aux_par (got {what})")
    if image is None or cls_label is None:
        raise _C.CosaError("export_refine: the image and the image-level label row are needed")
    _C.require_cuda(image, cam, cam_aux, cls_label, out)
    if image.dim() not in (3, 4) or image.numel() != 3 * image.shape[-2] * image.shape[-1] or image.shape[-3] != 3:
        raise ValueError(f"export_refine: image must be one image's [3,H,W], got {tuple(image.shape)}")
    H, W = int(image.shape[-2]), int(image.shape[-1])
    prep = lambda t: t.contiguous().float() if t is not None else None
    image, cam, cam_aux, cls = prep(image), prep(cam), prep(cam_aux), prep(cls_label)
    C = cls.numel()
    ref = cam if cam is not None else cam_aux
    if ref is None:
        raise _C.CosaError("export_refine: no CAM given")
    S = ref.shape[-1]
    for t, nm in ((cam, "cam"), (cam_aux, "cam_aux")):
        if t is not None and (t.numel() != C * S * S or tuple(t.shape[-3:]) != (C, S, S)):
            raise ValueError(f"export_refine: {nm} must be one image's [{C},{S},{S}], got {tuple(t.shape)}")
    if k_live is None:
        k_live = int((cls != 0).sum())
    offs, nbytes = export_record_layout(C, H, W, k_live, mask)
    if out is None:
        out = torch.empty(nbytes, device=image.device, dtype=torch.uint8)
    elif out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() < nbytes:
        raise ValueError(f"export_refine: `out` must be a contiguous uint8 record of at least {nbytes} bytes")
    L = _C.lib()
    dil = [int(d) for d in dilations]
    need = L.cosa_export_refine_workspace_bytes(H, W, int(k_live), mask, int(downscale or 0), len(dil))
    ws = _C.workspace(need, image.device, "export_par")        # need == 0: arguments the entry itself refuses, with its own message
    _C.check(L.cosa_export_refine(_C.ptr(image), _C.ptr(cam), _C.ptr(cam_aux), _C.ptr(cls), C, S, H, W, int(k_live), mask, float(high_thre),
                                  float(low_thre), int(ignore_index), int(downscale or 0), _C.int_array(dil), len(dil), int(num_iter),
                                  _C.ptr(out), out.numel(), _C.ptr(ws), ws.numel(), _C.stream_ptr()), "cosa_export_refine")
    return {k: out[o:o + H * W].reshape(H, W) for k, o in offs.items() if k in ("pseudo_par", "pseudo_aux_par")}


PREDICT_MAX_CLASSES = _C.constant("COSA_PREDICT_MAX_CLASSES")


def cls_threshold_logit(cls_thre):
    """the logit L a class must reach for a probability threshold t in (0, 1): float32(log(t / (1 - t))), formed in float64 on the host"""
    t = float(cls_thre)
    if not 0.0 < t < 1.0:
        raise ValueError(f"cls_thre must lie in (0, 1), got {cls_thre}")
    return float(np.float32(np.log(np.float64(t) / (np.float64(1.0) - np.float64(t)))))


def predict_classes(logits, cls_thre=0.5, cls_min=1, out=None):
    """The image-level class rows from the classification logits [G, C] (cosa_predict_classes): class c is present
    iff logit_c >= cls_threshold_logit(cls_thre); with fewer than `cls_min` present, the largest remaining logits are added (equal ones
    in index order; never a NaN or -inf).  -> (rows [G, C] fp32 in {0, 1}, k_live [G] int32, nonfinite [G] int32: the NaN / +-inf logits).
    `out`: the three tensors to write into (a caller that keeps them between calls).  No host wait."""
    _C.require_cuda(logits)
    if logits.dim() != 2:
        raise ValueError(f"predict_classes: logits must be [G, C], got {tuple(logits.shape)}")
    L = cls_threshold_logit(cls_thre)
    x = logits.contiguous().float()
    G, C = int(x.shape[0]), int(x.shape[1])
    if out is None:
        out = (torch.empty((G, C), device=x.device, dtype=torch.float32), torch.empty(G, device=x.device, dtype=torch.int32),
               torch.empty(G, device=x.device, dtype=torch.int32))
    rows, k_live, nonfinite = out
    _C.require_cuda(rows, k_live, nonfinite)
    if (rows.dtype, k_live.dtype, nonfinite.dtype) != (torch.float32, torch.int32, torch.int32) or rows.shape != (G, C) or \
            k_live.numel() != G or nonfinite.numel() != G or not (rows.is_contiguous() and k_live.is_contiguous() and nonfinite.is_contiguous()):
        raise ValueError("predict_classes: `out` must be contiguous (fp32 [G, C], int32 [G], int32 [G])")
    _C.check(_C.lib().cosa_predict_classes(_C.ptr(x), G, C, L, int(cls_min), _C.ptr(rows), _C.ptr(k_live), _C.ptr(nonfinite), _C.stream_ptr()),
             "cosa_predict_classes")
    return rows, k_live, nonfinite


_OVERLAY_PALETTE = {}                                    # str(device) -> the 256 x 3 colour map there


def overlay_alpha256(alpha):
    a = float(alpha)
    if not 0.0 <= a <= 1.0:
        raise ValueError(f"overlay alpha must lie in [0, 1], got {alpha}")
    return int(round(a * 256))


def export_overlay(image, seg, alpha=0.5, out=None, palette=None):
    """The label map `seg` (uint8 [H,W] or its H W bytes, e.g. a record's seg slot) painted over its image [3,H,W] / [1,3,H,W] (normalised
    fp32, as the loaders give it) with the colours of export_io.voc_colormap: label 0 keeps the image's byte, label l > 0 gives
    (a pal[l] + (256 - a) img + 128) >> 8 with a = round(alpha 256) (cosa_export_overlay).  `out`: 3 H W uint8 bytes to write into (a
    slice of the image's record).  -> uint8 [H, W, 3], a view of `out`."""
    _C.require_cuda(image, seg, out, palette)
    if image.dim() not in (3, 4) or image.shape[-3] != 3 or image.numel() != 3 * image.shape[-2] * image.shape[-1]:
        raise ValueError(f"export_overlay: image must be one image's [3,H,W], got {tuple(image.shape)}")
    H, W = int(image.shape[-2]), int(image.shape[-1])
    image = image.contiguous().float()
    if seg.dtype != torch.uint8 or seg.numel() != H * W or not seg.is_contiguous():
        raise ValueError(f"export_overlay: seg must be contiguous uint8 with {H * W} elements, got {seg.dtype} {tuple(seg.shape)}")
    if palette is None:
        palette = _OVERLAY_PALETTE.get(str(image.device))
        if palette is None:
            from .export_io import voc_colormap
            palette = _OVERLAY_PALETTE[str(image.device)] = torch.from_numpy(voc_colormap()).to(image.device)
    if palette.dtype != torch.uint8 or palette.numel() != 768 or not palette.is_contiguous():
        raise ValueError("export_overlay: the palette is 256 x 3 contiguous uint8")
    if out is None:
        out = torch.empty(3 * H * W, device=image.device, dtype=torch.uint8)
    elif out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() < 3 * H * W:
        raise ValueError(f"export_overlay: `out` must be contiguous uint8 of at least {3 * H * W} bytes")
    _C.check(_C.lib().cosa_export_overlay(_C.ptr(image), _C.ptr(seg), _C.ptr(palette), H, W, overlay_alpha256(alpha), _C.ptr(out),
                                          _C.stream_ptr()), "cosa_export_overlay")
    return out.reshape(-1)[:3 * H * W].reshape(H, W, 3)


CAMHEAT_MAX_CLASSES = _C.constant("COSA_CAMHEAT_MAX_CLASSES")
PANEL_COLOUR = (10, 186, 181)                            # the panel's region colour (csrc/heat_kernels.hip)


def _one_image(image, who):
    if image.dim() not in (3, 4) or image.shape[-3] != 3 or image.numel() != 3 * image.shape[-2] * image.shape[-1]:
        raise ValueError(f"{who}: image must be one image's [3,H,W], got {tuple(image.shape)}")
    return int(image.shape[-2]), int(image.shape[-1]), image.contiguous().float()


def export_camheat(planes, image, out=None):
    """The class planes `planes` (fp32 [k,H,W], e.g. a record's rawcam / rawcam_aux slot) as k heat maps over their image [3,H,W] /
    [1,3,H,W] (normalised fp32, as the loaders give it), in integers (cosa_export_camheat): idx = trunc(255 m)
    clamped to 0..255, the ramp (clamp(765 - |8 idx - k_c|, 0, 510) + 1) >> 1, plus the image's byte, times 255 over the picture's
    maximum.  `out`: at least 3 k H W uint8 bytes to write into (a slice of the image's record).  Two launches whatever k is, no host
    wait.  -> uint8 [k, H, W, 3], a view of `out`."""
    _C.require_cuda(planes, image, out)
    H, W, image = _one_image(image, "export_camheat")
    if planes.dtype != torch.float32 or planes.dim() != 3 or tuple(planes.shape[1:]) != (H, W) or not planes.is_contiguous():
        raise ValueError(f"export_camheat: planes must be contiguous fp32 [k,{H},{W}], got {planes.dtype} {tuple(planes.shape)}")
    k = int(planes.shape[0])
    if not 1 <= k <= CAMHEAT_MAX_CLASSES:
        raise ValueError(f"export_camheat: k must be in 1..{CAMHEAT_MAX_CLASSES} (got {k})")
    n = 3 * k * H * W
    if out is None:
        out = torch.empty(n, device=image.device, dtype=torch.uint8)
    elif out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() < n:
        raise ValueError(f"export_camheat: `out` must be contiguous uint8 of at least {n} bytes")
    ws = _C.workspace(4 * k, image.device, "camheat")
    _C.check(_C.lib().cosa_export_camheat(_C.ptr(planes), _C.ptr(image), k, H, W, _C.ptr(out), out.numel(), _C.ptr(ws), ws.numel(),
                                          _C.stream_ptr()), "cosa_export_camheat")
    return out.reshape(-1)[:n].reshape(k, H, W, 3)


def export_panel(heat, seg, class_idx, image, gt=None, out=None):
    """One comparison panel per class (cosa_export_panel), columns left to right: heat[j] (uint8 [k,H,W,3],
    export_camheat's pictures) | PANEL_COLOUR where seg == class_idx[j] + 1 | the same for gt (left out when `gt` is None; a gt of 255
    never matches) | the image.  seg, gt: contiguous uint8 with H W elements; class_idx: int32 [k] on the device, 0-based (a record's
    rawcam_idx slot).  `out`: at least 3 k H cols W bytes.  One launch.  -> uint8 [k, H, cols W, 3], cols = 4 with gt, else 3."""
    _C.require_cuda(heat, seg, class_idx, image, gt, out)
    H, W, image = _one_image(image, "export_panel")
    if heat.dtype != torch.uint8 or heat.dim() != 4 or tuple(heat.shape[1:]) != (H, W, 3) or not heat.is_contiguous():
        raise ValueError(f"export_panel: heat must be contiguous uint8 [k,{H},{W},3], got {heat.dtype} {tuple(heat.shape)}")
    k = int(heat.shape[0])
    if not 1 <= k <= CAMHEAT_MAX_CLASSES:
        raise ValueError(f"export_panel: k must be in 1..{CAMHEAT_MAX_CLASSES} (got {k})")
    for t, nm in ((seg, "seg"), (gt, "gt")):
        if t is not None and (t.dtype != torch.uint8 or t.numel() != H * W or not t.is_contiguous()):
            raise ValueError(f"export_panel: {nm} must be contiguous uint8 with {H * W} elements, got {t.dtype} {tuple(t.shape)}")
    if class_idx.dtype != torch.int32 or class_idx.numel() != k or not class_idx.is_contiguous():
        raise ValueError(f"export_panel: class_idx must be contiguous int32 [{k}], got {class_idx.dtype} {tuple(class_idx.shape)}")
    cols = 4 if gt is not None else 3
    n = 3 * k * H * cols * W
    if out is None:
        out = torch.empty(n, device=image.device, dtype=torch.uint8)
    elif out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() < n:
        raise ValueError(f"export_panel: `out` must be contiguous uint8 of at least {n} bytes")
    _C.check(_C.lib().cosa_export_panel(_C.ptr(heat), _C.ptr(seg), _C.ptr(gt), _C.ptr(class_idx), _C.ptr(image), k, H, W, _C.ptr(out),
                                        out.numel(), _C.stream_ptr()), "cosa_export_panel")
    return out.reshape(-1)[:n].reshape(k, H, cols * W, 3)


# --------------------------------------------------------------------------------------------
# cam_validation / cam2mask  (utils/seg_helper.py:547-551, 721-797)
# --------------------------------------------------------------------------------------------
def cam_validation(cam, cls_label):
    """utils/seg_helper.py:547-551 (broadcast multiply; no materialised repeat)."""
    return cam * cls_label[:, :, None, None]


def _boxes_to_device(img_boxes, device):
    if not torch.is_tensor(img_boxes):
        img_boxes = torch.as_tensor(img_boxes)
    return img_boxes.to(device=device, dtype=torch.int32, non_blocking=True).contiguous()


def cam2mask(images, img_boxes, cams, cls_labels, threshold_high, threshold_low, refine_model=None, ignore_index=255,
             downscale=2, _fold_validation=False):
    """CAM -> {0..C, 255} label mask [b,h,w] (float32), one fused launch sequence for the whole batch.

    utils/seg_helper.py:721-785 (+ _refine_cams :787-797).  `refine_model` may be None (reference
    default) or a cosa_amd.models.PAR.PAR instance (the reference's only refine model).
    `cams` are the validated CAMs as in the reference call order (main.py:137,158-166);
    `_fold_validation=True` lets the training loop pass raw CAMs and skip cam_validation's pass.
    """
    return cam2mask_multi(images, img_boxes, [cams], cls_labels, [threshold_high], [threshold_low], refine_model=refine_model,
                          ignore_index=ignore_index, downscale=downscale, _fold_validation=_fold_validation)[0]


def _cam2mask_generic(images, img_boxes, cams, cls_labels, threshold_high, threshold_low, refine_model, ignore_index, downscale):
    """utils/seg_helper.py:721-797 as written there (per-image loop, torch ops on the device), for what the fused kernels do not
    cover: an arbitrary callable `refine_model`, non-square crops, other downscale factors.  `cams` are the validated CAMs."""
    b, _, h, w = images.shape
    dev = cams.device
    size = [h // downscale, w // downscale] if downscale else None
    rs = (lambda t: F.interpolate(t, size=size, mode="bilinear", align_corners=False)) if downscale else (lambda t: t)
    _images = rs(images.float())
    plane = torch.ones((b, 1, h, w), device=dev)
    hi = torch.as_tensor(threshold_high, device=dev, dtype=torch.float32)
    lo = torch.as_tensor(threshold_low, device=dev, dtype=torch.float32)
    cams_h, cams_l = rs(torch.cat([plane * hi, cams], dim=1)), rs(torch.cat([plane * lo, cams], dim=1))
    with_bkg = torch.cat([torch.ones((b, 1), device=dev), cls_labels.float()], dim=1)
    out_h = torch.full((b, h, w), float(ignore_index), device=dev)
    out_l = out_h.clone()

    def refine(img, act, keys):
        r = refine_model(img, act) if refine_model is not None else act
        r = F.interpolate(r, size=(h, w), mode="bilinear", align_corners=False)
        return keys[r.argmax(dim=1)]

    boxes = torch.as_tensor(img_boxes).tolist()
    for i, (y0, y1, x0, x1) in enumerate(boxes):
        keys = torch.nonzero(with_bkg[i])[:, 0]
        out_h[i, y0:y1, x0:x1] = refine(_images[[i]], cams_h[i, keys].unsqueeze(0).softmax(dim=1), keys)[0, y0:y1, x0:x1].float()
        out_l[i, y0:y1, x0:x1] = refine(_images[[i]], cams_l[i, keys].unsqueeze(0).softmax(dim=1), keys)[0, y0:y1, x0:x1].float()
    mask = out_h.clone()
    mask[out_h == 0] = ignore_index
    mask[(out_h + out_l) == 0] = 0
    return mask


_BOX_SIZE_CACHE = {}       # (h, w, device, dtype) -> [h, h, w, w] on that device (cam2mask_multi: negative box bounds)


def cam2mask_multi(images, img_boxes, cams_list, cls_labels, thresholds_high, thresholds_low, refine_model=None, ignore_index=255,
                   downscale=2, _fold_validation=False):
    """cam2mask for several CAM sets of the SAME images (the training step's main and auxiliary CAMs, main.py:137-166) in
    one pass: the refine model's affinities are built once and streamed once per propagation step for all sets.  Returns
    a list of label maps, each bit-identical to a separate cam2mask call."""
    G = len(cams_list)
    if not (G >= 1 and len(thresholds_high) == G and len(thresholds_low) == G):
        raise ValueError("cam2mask_multi: one (high, low) threshold pair per CAM set")
    _C.require_cuda(cls_labels, *cams_list)
    b, _, h, w = images.shape
    generic = (refine_model is not None and not isinstance(refine_model, PAR)) or h != w or downscale not in (0, 2, None, False)
    if generic:
        # any other callable refine model (the reference accepts whatever `refine_model(images, cams)` returns,
        # utils/seg_helper.py:787-792), non-square crops and other downscale factors: the reference's per-image loop on the GPU
        if refine_model is not None and not callable(refine_model):
            raise TypeError("cam2mask: refine_model must be None or a callable (images[1,3,h,w], cams[1,K,h,w]) -> [1,K,h',w']")
        return [_cam2mask_generic(images, img_boxes, c.float() * cls_labels[:, :, None, None] if _fold_validation else c.float(),
                                  cls_labels, th, tl, refine_model, ignore_index, downscale)
                for c, th, tl in zip(cams_list, thresholds_high, thresholds_low)]
    downscale = 2 if downscale == 2 else 0
    cams_list = [c.contiguous().float() for c in cams_list]
    cls_labels = cls_labels.contiguous().float()
    C = cams_list[0].shape[1]
    for c in cams_list:
        if c.shape != (b, C, h, w) or cls_labels.shape != (b, C):
            raise ValueError("cam2mask: cams must be [b,C,h,w] at image size and cls_labels [b,C]")
    dev = cams_list[0].device
    # the reference slices with the box (`mask[y0:y1, x0:x1]`, seg_helper.py:776-777), so negative bounds count from the end -- evaluation passes
    # [0, -1, 0, -1] (evaluation_engine.py:136): bring them to the kernels' absolute form (checked on the host when the boxes live there)
    if not torch.is_tensor(img_boxes):
        img_boxes = torch.as_tensor(img_boxes)
    if img_boxes.is_cuda or bool((img_boxes < 0).any()):
        key = (h, w, img_boxes.device, img_boxes.dtype)
        size = _BOX_SIZE_CACHE.get(key)
        if size is None:           # (built once per geometry: a fresh torch.tensor(..., device=cuda) is a pageable host-to-device copy on every call)
            size = _BOX_SIZE_CACHE[key] = torch.tensor([h, h, w, w], device=img_boxes.device, dtype=img_boxes.dtype)
        img_boxes = torch.where(img_boxes < 0, img_boxes + size, img_boxes)
    boxes = _boxes_to_device(img_boxes, dev)
    if boxes.shape != (b, 4):
        raise ValueError("cam2mask: img_boxes must be [b,4]")
    masks = [torch.empty((b, h, w), device=dev, dtype=torch.float32) for _ in range(G)]
    L = _C.lib()
    if refine_model is not None:
        _C.require_cuda(images)
        images = images.contiguous().float()
        dil, nd, iters = _C.int_array(refine_model.dilations), len(refine_model.dilations), refine_model.num_iter
    else:
        dil, nd, iters = _C.int_array([1]), 0, 0
    ws = _C.workspace(L.cosa_cam2mask_multi_workspace_bytes(G, b, C, h, downscale, nd if iters > 0 else 0), dev, "cam2mask")
    cam_ptrs = (ctypes.c_void_p * G)(*[c.data_ptr() for c in cams_list])
    mask_ptrs = (ctypes.c_void_p * G)(*[m.data_ptr() for m in masks])
    on_device = any(torch.is_tensor(t) for t in list(thresholds_high) + list(thresholds_low))
    if on_device:
        # thresholds that live on the device (adaptive thresholds): [G][hi, lo] float32, read by the kernels -- no host sync
        tdev = torch.stack([torch.stack([torch.as_tensor(h, device=dev).reshape(()).to(torch.float32),
                                         torch.as_tensor(l, device=dev).reshape(()).to(torch.float32)])
                            for h, l in zip(thresholds_high, thresholds_low)]).contiguous()
        hi = lo = (ctypes.c_float * G)(*([0.0] * G))
    else:
        tdev = None
        hi = (ctypes.c_float * G)(*[float(t) for t in thresholds_high])
        lo = (ctypes.c_float * G)(*[float(t) for t in thresholds_low])
    _C.check(L.cosa_cam2mask_multi(_C.ptr(images if iters > 0 else None), _C.ptr(boxes), cam_ptrs, _C.ptr(cls_labels), mask_ptrs,
                                   hi, lo, _C.ptr(tdev), G, b, C, h, downscale, int(bool(_fold_validation)), dil, nd, iters, float(ignore_index),
                                   _C.ptr(ws), ws.numel(), _C.stream_ptr()), "cosa_cam2mask_multi")
    return masks


# --------------------------------------------------------------------------------------------
# adaptive thresholds  (utils/seg_helper.py:924-959, main.py:94-103,138-151,174-184)
# --------------------------------------------------------------------------------------------
class DynamicQueue(object):
    """utils/seg_helper.py:946-959 with the storage on the device: a ring of `max_size` rows x `dim` float64 values, created
    with uniform noise exactly as the reference's is (np.random.random) and overwritten `batch_size` rows at a time."""

    def __init__(self, max_size, dim, batch_size, device="cuda"):
        self.max_size = max_size
        self.queue = torch.from_numpy(np.random.random((max_size, dim))).to(device)
        self.ptr = 0
        self.batch_size = batch_size

    def update(self, income):
        # income -> batchsize,dim (device tensor, any float dtype; stored as float64 like the reference's numpy queue)
        self.queue[self.ptr:self.ptr + self.batch_size, :] = income.reshape(self.batch_size, -1).to(self.queue.dtype)
        self.ptr = (self.ptr + self.batch_size) % self.max_size

    def getqueue(self):
        return self.queue


def cell_bilinear(x, g):
    """F.interpolate(x, size=(g, g), mode='bilinear', align_corners=False) for an integer, even reduction factor (main.py:140:
    448 -> 28): every output is 0.5*(0.5*a + 0.5*b) + 0.5*(0.5*c + 0.5*d) of the four pixels around the cell centre, evaluated
    in ATen's order, so the values are bit-identical -- but as four strided gathers instead of ATen's kernel, which gives a
    whole [b*C] column to each of only g*g threads (0.74 ms per call at b=16, C=20; this: ~30 us)."""
    S = x.shape[-1]
    s = S // g if g > 0 else 0
    if x.shape[-2] != S or g <= 0 or s * g != S or s % 2:
        return F.interpolate(x, size=(g, g), mode='bilinear', align_corners=False)
    a = s // 2 - 1
    r0, r1 = x[:, :, a::s, :], x[:, :, a + 1::s, :]
    top = 0.5 * r0[..., a::s] + 0.5 * r0[..., a + 1::s]
    bot = 0.5 * r1[..., a::s] + 0.5 * r1[..., a + 1::s]
    return 0.5 * top + 0.5 * bot


def rungmm_device(queue, modal, filter_thre=0.05, tol=1e-3, reg_covar=1e-6, max_iter=100):
    """The fit of `rungmm` without leaving the device: returns a float64 tensor [13] -- [0] low threshold (largest sample of
    component 0), [1] high threshold (smallest sample of component 2; NaN for modal=2), [2] EM iterations, [3] status bits
    (see include/cosa_hip.h), then means / weights / inverse sigmas.  No host synchronisation."""
    assert modal in [2, 3]
    if filter_thre < 0:
        raise ValueError("rungmm: filter_thre must be >= 0")
    _C.require_cuda(queue)
    q = queue.to(torch.float64).flatten()
    keep = q > filter_thre
    xs, _ = torch.sort(torch.where(keep, q, torch.full_like(q, float("inf"))))
    n = keep.sum()                                                   # int64, stays on the device
    out = torch.empty(13, device=q.device, dtype=torch.float64)
    L = _C.lib()
    ws = _C.workspace(L.cosa_gmm_workspace_bytes(), q.device, "gmm")
    _C.check(L.cosa_gmm_fit_thresholds(_C.ptr(xs), _C.ptr(n), xs.numel(), modal, tol, reg_covar, max_iter, _C.ptr(out), _C.ptr(ws),
                                       ws.numel(), _C.stream_ptr()), "cosa_gmm_fit_thresholds")
    return out


def rungmm(queue, modal, filter_thre=0.05):
    """utils/seg_helper.py:924-943: (low, high) for modal=3, low for modal=2, as Python floats (this form synchronises; the
    training step uses rungmm_device).  An empty outer component raises ValueError like the reference's max() / min()."""
    if isinstance(queue, np.ndarray):
        queue = torch.from_numpy(queue).cuda()
    out = rungmm_device(queue, modal, filter_thre).tolist()
    status = int(out[3])
    if status & 8:
        raise _C.CosaError("rungmm: device barrier expired")
    if status & 4:
        raise ValueError("rungmm: fewer samples above filter_thre than mixture components")
    if status & 1 or (modal == 3 and status & 2):
        raise ValueError("rungmm: max()/min() of an empty component")
    return out[0] if modal == 2 else (out[0], out[1])


# --------------------------------------------------------------------------------------------
# seg_loss  (utils/seg_helper.py:800-813)
# --------------------------------------------------------------------------------------------
def seg_loss(seg_pred, mask_label, fg_alpha=0.5, ignore_index=255):
    assert fg_alpha >= 0 and fg_alpha <= 1, "fg_alpha should be in [0,1]"
    lab = mask_label.long()
    bg_label = torch.where(lab != 0, torch.full_like(lab, ignore_index), lab)
    fg_label = torch.where(lab == 0, torch.full_like(lab, ignore_index), lab)
    # one log-softmax pass shared by the two class-balanced terms
    logp = F.log_softmax(seg_pred.float(), dim=1)
    bg_loss = F.nll_loss(logp, bg_label, ignore_index=ignore_index, reduction='sum') / ((bg_label != ignore_index).sum() + 1e-6)
    fg_loss = F.nll_loss(logp, fg_label, ignore_index=ignore_index, reduction='sum') / ((fg_label != ignore_index).sum() + 1e-6)
    return (1 - fg_alpha) * bg_loss + fg_alpha * fg_loss


# --------------------------------------------------------------------------------------------
# DenseEnergyLoss  (utils/seg_helper.py:191-230, 864-903)
# --------------------------------------------------------------------------------------------
class DenseEnergyLossFunction(Function):
    """utils/seg_helper.py:864-903 with the bilateral filter, gate, dot product and the backward
    scaling all on the device (no D2H/H2D hops, no host-side AS)."""

    @staticmethod
    def forward(ctx, images, segmentations, sigma_rgb, sigma_xy, ROIs, unlabel_region):
        _C.require_cuda(images, segmentations, ROIs, unlabel_region)
        N, K, H, W = segmentations.shape
        images = images.contiguous().float()
        seg = segmentations.contiguous().float()
        roi = ROIs.contiguous().float()
        unl = unlabel_region.contiguous().to(torch.uint8)
        AS = torch.empty_like(seg)
        loss = torch.empty(1, device=seg.device, dtype=torch.float32)
        L = _C.lib()
        ws = _C.workspace(L.cosa_bilateral_workspace_bytes(N, K, H, W), seg.device, "bilateral")
        _C.check(L.cosa_dense_energy_forward(_C.ptr(images), _C.ptr(seg), _C.ptr(roi), _C.ptr(unl), _C.ptr(AS), _C.ptr(loss),
                                             N, K, H, W, float(sigma_rgb), float(sigma_xy), _C.ptr(ws), ws.numel(),
                                             _C.stream_ptr()), "cosa_dense_energy_forward")
        ctx.save_for_backward(AS, roi)
        ctx.shape = (N, K, H, W)
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        AS, roi = ctx.saved_tensors
        N, K, H, W = ctx.shape
        g = grad_output.contiguous().float()
        grad_seg = torch.empty_like(AS)
        _C.check(_C.lib().cosa_dense_energy_backward(_C.ptr(AS), _C.ptr(roi), _C.ptr(g), _C.ptr(grad_seg), N, K, H, W,
                                                     _C.stream_ptr()), "cosa_dense_energy_backward")
        return None, grad_seg, None, None, None, None


class DenseEnergyLoss(torch.nn.Module):
    """utils/seg_helper.py:191-208"""

    def __init__(self, weight, sigma_rgb, sigma_xy, scale_factor):
        super().__init__()
        self.weight = weight
        self.sigma_rgb = sigma_rgb
        self.sigma_xy = sigma_xy
        self.scale_factor = scale_factor

    def forward(self, images, segmentations, ROIs, seg_label):
        sf = self.scale_factor
        scaled_images = F.interpolate(images, scale_factor=sf, recompute_scale_factor=True)
        scaled_segs = F.interpolate(segmentations, scale_factor=sf, mode='bilinear', align_corners=False,
                                    recompute_scale_factor=True)
        scaled_ROIs = F.interpolate(ROIs.unsqueeze(1), scale_factor=sf, recompute_scale_factor=True).squeeze(1)
        scaled_seg_label = F.interpolate(seg_label.float(), scale_factor=sf, mode='nearest', recompute_scale_factor=True)
        unlabel_region = (scaled_seg_label.long() == 255).squeeze(1)
        return self.weight * DenseEnergyLossFunction.apply(scaled_images, scaled_segs, self.sigma_rgb,
                                                           self.sigma_xy * self.scale_factor, scaled_ROIs, unlabel_region)

    def extra_repr(self):
        return 'sigma_rgb={}, sigma_xy={}, weight={}, scale_factor={}'.format(
            self.sigma_rgb, self.sigma_xy, self.weight, self.scale_factor)


def seg_blend_weights(fg_alpha=0.5, aux_alpha=0.5, has_aux=True):
    """(wA_bg, wA_fg, wB_bg, wB_fg): the weights of the four class-balanced terms of main.py:200-203 x seg_helper.py:813,
    (1-b) ((1-a) bgA + a fgA) + b ((1-a) bgB + a fgB) with a = fg_alpha (--segfg_alpha), b = aux_alpha (--aux_cam2seg_alpha); without an
    auxiliary label map (--aux_cam2seg false) b = 0.  The reference asserts a in [0, 1] (seg_helper.py:803); b outside [0, 1] would make a
    weight negative, which the kernels' fixed-point range argument does not cover: refused here, as the entry point would."""
    a, b = float(fg_alpha), (float(aux_alpha) if has_aux else 0.0)
    if not (0.0 <= a <= 1.0):
        raise ValueError(f"fg_alpha {fg_alpha!r} should be in [0,1]")
    if not (0.0 <= b <= 1.0):
        raise ValueError(f"aux_alpha {aux_alpha!r} should be in [0,1]")
    return ((1 - b) * (1 - a), (1 - b) * a, b * (1 - a), b * a)


_DEFAULT_BLEND = (0.25, 0.25, 0.25, 0.25)
_blend_vecs = {}


def _blend_vec(weights, device):
    """the four weights as a device vector, made once per (setting, device)"""
    key = (weights, str(device))
    v = _blend_vecs.get(key)
    if v is None:
        v = _blend_vecs[key] = torch.tensor(weights, device=device, dtype=torch.float32)
    return v


def _rel_pair(rel_main, rel_aux, mask_aux):
    """(relA, relB | None) for the _rw entry points, or None without weight maps: one map per label map"""
    if rel_main is None:
        if rel_aux is not None:
            raise ValueError("seg loss: rel_aux without rel_main")
        return None
    if (rel_aux is None) != (mask_aux is None):
        raise ValueError("seg loss: an auxiliary weight map goes with an auxiliary label map, and only with one")
    return (rel_main, rel_aux)


def _seg_loss_launch(seg_lr, maskA, maskB, simg, boxes, weights, rel=None):
    """the seg-loss forward kernel -> (its eight sums, (seg_lr, maskA, maskB) as the kernel read them, (s_seg, s_img, roi, unlabel): the
    half-resolution tensors it leaves for the regulariser).  `weights`: FusedSegRegLoss's.  `rel` = (relA, relB | None): per-pixel weight
    maps [B,S,S] fp32 beside the label maps, contiguous on the device -- the call then goes to cosa_seg_loss_forward_rw."""
    _C.require_cuda(seg_lr, maskA, maskB, simg, boxes)
    if maskB is None and (weights is None or weights[2] != 0 or weights[3] != 0):
        raise ValueError("FusedSegRegLoss: no auxiliary label map needs weights with wB_bg = wB_fg = 0")
    seg_lr = seg_lr.contiguous().float()
    B, K, hs, ws = seg_lr.shape
    S = maskA.shape[-1]
    Sq = S // 2
    dev = seg_lr.device
    sums = torch.empty(8, device=dev)
    s_seg = torch.empty((B, K, Sq, Sq), device=dev)
    s_img = torch.empty((B, 3, Sq, Sq), device=dev)
    roi = torch.empty((B, Sq, Sq), device=dev)
    unl = torch.empty((B, Sq, Sq), device=dev, dtype=torch.uint8)
    L = _C.lib()
    maskA, simg = maskA.contiguous().float(), simg.contiguous().float()
    maskB = maskB.contiguous().float() if maskB is not None else None
    wsl = _C.workspace(L.cosa_seg_loss_workspace_bytes(B, K, hs, ws), dev, "seg_loss")
    if rel is None:
        fwd_name, tail = ("cosa_seg_loss_forward" if weights is None else "cosa_seg_loss_forward_w"), ()
    else:
        if weights is None:
            raise ValueError("FusedSegRegLoss: weight maps need `weights` (the entry points with the defaults built in take none)")
        _C.require_cuda(*rel)
        for r, m in zip(rel, (maskA, maskB)):
            if r is not None and (r.shape != m.shape or r.dtype != torch.float32 or not r.is_contiguous()):
                raise ValueError("FusedSegRegLoss: a weight map is contiguous fp32 of its label map's shape")
        fwd_name, tail = "cosa_seg_loss_forward_rw", (_C.ptr(rel[0]), _C.ptr(rel[1]))
    _C.check(getattr(L, fwd_name)(_C.ptr(seg_lr), _C.ptr(maskA), _C.ptr(maskB), _C.ptr(simg), _C.ptr(boxes), _C.ptr(sums),
                                  _C.ptr(s_seg), _C.ptr(s_img), _C.ptr(roi), _C.ptr(unl), B, K, hs, ws, S, _C.ptr(wsl), wsl.numel(),
                                  _C.stream_ptr(), *tail), fwd_name)
    return sums, (seg_lr, maskA, maskB), (s_seg, s_img, roi, unl)


def _seg_loss_value(sums, weights):
    """the seg loss from the forward kernel's eight sums: 0.5 * (0.5 bgA + 0.5 fgA) + 0.5 * (0.5 bgB + 0.5 fgB), each term sum / (count + 1e-6)
    (seg_helper.py:800-813, main.py:200-203), or the same with FusedSegRegLoss's `weights`: four vector ops instead of eighteen scalar ones"""
    pairs = sums.view(4, 2)
    if weights is None or tuple(weights) == _DEFAULT_BLEND:
        return (pairs[:, 0] / (pairs[:, 1] + 1e-6)).sum() * 0.25
    # sum_i w_i sums_i / (cnt_i + 1e-6); a group without a pixel (and all of B without a second map) is 0 / 1e-6 = 0
    return ((pairs[:, 0] / (pairs[:, 1] + 1e-6)) * _blend_vec(tuple(weights), sums.device)).sum()


class FusedSegRegLoss(Function):
    """seg_loss(main) / seg_loss(aux) blend + dense-energy regulariser of the SAME low-res logits in two launches.

    Equivalent to main.py:167-212 (F.interpolate -> seg_loss x2 -> get_energy_loss), but nothing of size [b,K,S,S] is ever written: the
    kernels re-derive the per-pixel softmax from an LDS tile of the low-res logits.  Returns (seg_loss, reg_loss).
    `weights` = None: fg_alpha = 0.5 and aux_cam2seg_alpha = 0.5 (the reference defaults) through the entry points that have these built in
    (maskB required).  `weights` = seg_blend_weights(...): the general entry points (cosa_seg_loss_*_w); maskB may then be None (no auxiliary
    label map).  Both give the same bits for the defaults (tests/test_loss_flags_gpu.py).
    `rel` = (relA, relB | None): per-pixel weight maps beside the label maps (seg_weightloss) through the _rw entry
    points; None: the calls above, untouched."""

    @staticmethod
    def forward(ctx, seg_lr, maskA, maskB, simg, boxes, weight, sigma_rgb, sigma_xy, prepared=None, weights=None, rel=None):
        sums, (seg_lr, maskA, maskB), (s_seg, s_img, roi, unl) = _seg_loss_launch(seg_lr, maskA, maskB, simg, boxes, weights, rel)
        B, K, Sq = s_seg.shape[0], s_seg.shape[1], s_seg.shape[-1]
        S = maskA.shape[-1]
        dev = seg_lr.device
        L = _C.lib()
        AS = torch.empty_like(s_seg)
        energy = torch.empty(1, device=dev)
        if prepared is not None and prepared.matches(B, K, Sq, sigma_rgb, sigma_xy):
            # the lattice of this strong image was built on a side stream while the networks ran (PreparedLattice)
            prepared.join()
            _C.check(L.cosa_dense_energy_forward_prepared(_C.ptr(s_seg), _C.ptr(roi), _C.ptr(unl), _C.ptr(AS), _C.ptr(energy), B, K, Sq, Sq,
                                                          float(sigma_rgb), float(sigma_xy), _C.ptr(prepared.ws), prepared.ws.numel(),
                                                          _C.stream_ptr()), "cosa_dense_energy_forward_prepared")
        else:
            wsb = _C.workspace(L.cosa_bilateral_workspace_bytes(B, K, Sq, Sq), dev, "bilateral")
            _C.check(L.cosa_dense_energy_forward(_C.ptr(s_img), _C.ptr(s_seg), _C.ptr(roi), _C.ptr(unl), _C.ptr(AS), _C.ptr(energy), B, K,
                                                 Sq, Sq, float(sigma_rgb), float(sigma_xy), _C.ptr(wsb), wsb.numel(), _C.stream_ptr()),
                     "cosa_dense_energy_forward")
        seg_l = _seg_loss_value(sums, weights)      # (after the energy launches, which hide its five small ops: in front of them a step measured 0.27 ms more)
        ctx.save_for_backward(seg_lr, maskA, maskB, sums, AS, roi, *(rel if rel is not None else ()))
        ctx.weights = None if weights is None else tuple(float(w) for w in weights)
        ctx.weight = float(weight)
        ctx.S = S
        return seg_l, energy * float(weight)

    @staticmethod
    def backward(ctx, g_seg, g_reg):
        seg_lr, maskA, maskB, sums, AS, roi, *rel = ctx.saved_tensors
        B, K, hs, ws = seg_lr.shape
        grad = torch.empty_like(seg_lr)
        gs = g_seg.reshape(1).float().contiguous()
        gr = (g_reg.reshape(1).float() * ctx.weight).contiguous()
        wsl = _C.workspace(_C.lib().cosa_seg_loss_workspace_bytes(B, K, hs, ws), seg_lr.device, "seg_loss")
        if rel:
            _C.check(_C.lib().cosa_seg_loss_backward_rw(_C.ptr(seg_lr), _C.ptr(maskA), _C.ptr(maskB), _C.ptr(sums), _C.ptr(AS), _C.ptr(roi),
                                                        _C.ptr(gs), _C.ptr(gr), _C.ptr(grad), *ctx.weights, B, K, hs, ws, ctx.S, _C.ptr(wsl),
                                                        wsl.numel(), _C.stream_ptr(), _C.ptr(rel[0]), _C.ptr(rel[1])), "cosa_seg_loss_backward_rw")
        elif ctx.weights is None:
            _C.check(_C.lib().cosa_seg_loss_backward(_C.ptr(seg_lr), _C.ptr(maskA), _C.ptr(maskB), _C.ptr(sums), _C.ptr(AS), _C.ptr(roi),
                                                     _C.ptr(gs), _C.ptr(gr), _C.ptr(grad), B, K, hs, ws, ctx.S, _C.ptr(wsl), wsl.numel(),
                                                     _C.stream_ptr()), "cosa_seg_loss_backward")
        else:
            _C.check(_C.lib().cosa_seg_loss_backward_w(_C.ptr(seg_lr), _C.ptr(maskA), _C.ptr(maskB), _C.ptr(sums), _C.ptr(AS), _C.ptr(roi),
                                                       _C.ptr(gs), _C.ptr(gr), _C.ptr(grad), *ctx.weights, B, K, hs, ws, ctx.S, _C.ptr(wsl),
                                                       wsl.numel(), _C.stream_ptr()), "cosa_seg_loss_backward_w")
        return grad, None, None, None, None, None, None, None, None, None, None


class PreparedLattice:
    """The image-only half of the dense-energy regulariser (half-resolution de-normalised strong image + permutohedral lattice:
    hash table, per-pixel offsets / weights, blur neighbours) built on a side stream at the start of a step, so that only splat /
    blur / slice wait for the student's logits.  One instance per trainer; `start(simg, K)` then pass it to
    fused_seg_and_energy_loss(..., prepared=...)."""

    def __init__(self, sigma_rgb, sigma_xy):
        self.sigma = (float(sigma_rgb), float(sigma_xy))
        self.stream = None
        self.event = None
        self.ws = self.s_img = None
        self.key = None

    def start(self, simg, K):
        _C.require_cuda(simg)
        B, _, S, _ = simg.shape
        dev = simg.device
        if self.stream is None:
            self.stream, self.event = torch.cuda.Stream(device=dev), torch.cuda.Event()
        L = _C.lib()
        need = L.cosa_bilateral_workspace_bytes(B, K, S // 2, S // 2)
        if self.ws is None or self.ws.numel() < need or self.ws.device != dev:
            self.ws = torch.empty(need, device=dev, dtype=torch.uint8)
        if self.s_img is None or self.s_img.shape != (B, 3, S // 2, S // 2):
            self.s_img = torch.empty((B, 3, S // 2, S // 2), device=dev, dtype=torch.float32)
        simg = simg.contiguous().float()
        self.stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(self.stream):
            _C.check(L.cosa_dense_energy_prepare(_C.ptr(simg), _C.ptr(self.s_img), B, K, S, self.sigma[0], self.sigma[1], _C.ptr(self.ws),
                                                 self.ws.numel(), _C.stream_ptr()), "cosa_dense_energy_prepare")
            self.event.record(self.stream)
        simg.record_stream(self.stream)
        self.key = (B, K, S // 2)

    def matches(self, B, K, Sq, sigma_rgb, sigma_xy):
        return self.key == (B, K, Sq) and self.sigma == (float(sigma_rgb), float(sigma_xy))

    def join(self):
        torch.cuda.current_stream().wait_event(self.event)
        self.key = None                                  # one filter pass per prepared lattice in the training step


def fused_seg_and_energy_loss(seg_pred_lr, mask_main, mask_aux, img, img_box, loss_layer, prepared=None, fg_alpha=0.5, aux_alpha=0.5,
                              _builtin_defaults=False, rel_main=None, rel_aux=None):
    """(seg_loss, reg_loss) of main.py:167-212 for DenseEnergyLoss(scale_factor=0.5):
    (1 - aux_alpha) seg_loss(main, fg_alpha) + aux_alpha seg_loss(aux, fg_alpha), or seg_loss(main, fg_alpha) alone with `mask_aux` = None
    (--aux_cam2seg false), and the regulariser on the main labels.
    `prepared`: a PreparedLattice started on this step's `img` (optional; otherwise the lattice is built here).
    `_builtin_defaults`: the entry points with fg_alpha = aux_alpha = 0.5 built in instead of the weighted ones (same bits; kept for the
    test of exactly that).
    `rel_main` / `rel_aux`: per-pixel weight maps [b,S,S] fp32 in [0, 1] beside the label maps (label_reliability): each seg_loss term becomes
    seg_weightloss with its map, on the _rw entry points.  None: today's calls, untouched."""
    if loss_layer.scale_factor != 0.5:
        raise NotImplementedError("fused losses are built for DenseEnergyLoss(scale_factor=0.5) (main.py:77)")
    boxes = _boxes_to_device(img_box, seg_pred_lr.device)
    weights = seg_blend_weights(fg_alpha, aux_alpha, mask_aux is not None)
    if _builtin_defaults:
        if weights != _DEFAULT_BLEND:
            raise ValueError("_builtin_defaults: the built-in entry points are fg_alpha = aux_alpha = 0.5 with an auxiliary label map")
        weights = None
    return FusedSegRegLoss.apply(seg_pred_lr, mask_main, mask_aux, img, boxes, loss_layer.weight, loss_layer.sigma_rgb,
                                 loss_layer.sigma_xy * loss_layer.scale_factor, prepared, weights, _rel_pair(rel_main, rel_aux, mask_aux))


def _crop_mask_from_boxes(img_box, b, h, w, device):
    boxes = _boxes_to_device(img_box, device)
    ys = torch.arange(h, device=device, dtype=torch.int32)[None, :, None]
    xs = torch.arange(w, device=device, dtype=torch.int32)[None, None, :]
    inside = (ys >= boxes[:, 0, None, None]) & (ys < boxes[:, 1, None, None]) & \
             (xs >= boxes[:, 2, None, None]) & (xs < boxes[:, 3, None, None])
    return inside.float()


class SoftmaxHalfRes(Function):
    """F.softmax(logit, dim=1) followed by DenseEnergyLoss.forward's resize of the probabilities by 0.5 (utils/seg_helper.py:199-203, 224),
    forward and backward in one kernel each: nothing of the logits' size is written forward."""

    @staticmethod
    def forward(ctx, logit):
        logit = logit.contiguous().float()
        B, K, H, W = logit.shape
        out = torch.empty((B, K, H // 2, W // 2), device=logit.device, dtype=torch.float32)
        _C.check(_C.lib().cosa_softmax_halfres_forward(_C.ptr(logit), _C.ptr(out), B, K, H, W, _C.stream_ptr()), "cosa_softmax_halfres_forward")
        ctx.save_for_backward(logit)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (logit,) = ctx.saved_tensors
        B, K, H, W = logit.shape
        g = grad_out.contiguous().float()
        grad = torch.empty_like(logit)
        _C.check(_C.lib().cosa_softmax_halfres_backward(_C.ptr(logit), _C.ptr(g), _C.ptr(grad), B, K, H, W, _C.stream_ptr()),
                 "cosa_softmax_halfres_backward")
        return grad


def get_energy_loss(img, logit, label, img_box, loss_layer, mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375]):
    """utils/seg_helper.py:210-230 (box mask built with one broadcast compare instead of a Python loop).  With the reference's
    scale_factor = 0.5 on the GPU the softmax and the layer's resize of the probabilities are one kernel (SoftmaxHalfRes)."""
    b, _, h, w = logit.shape
    crop_mask = _crop_mask_from_boxes(img_box, b, h, w, logit.device)
    mean_t = torch.tensor(mean, device=img.device, dtype=torch.float32)[None, :, None, None]
    std_t = torch.tensor(std, device=img.device, dtype=torch.float32)[None, :, None, None]
    _img = img * std_t + mean_t
    seg_label = label.type(torch.uint8).unsqueeze(1)
    if logit.is_cuda and loss_layer.scale_factor == 0.5 and h % 2 == 0 and w % 2 == 0:
        sf = loss_layer.scale_factor
        scaled_segs = SoftmaxHalfRes.apply(logit)
        scaled_images = F.interpolate(_img, scale_factor=sf, recompute_scale_factor=True)
        scaled_ROIs = F.interpolate(crop_mask.unsqueeze(1), scale_factor=sf, recompute_scale_factor=True).squeeze(1)
        scaled_seg_label = F.interpolate(seg_label.float(), scale_factor=sf, mode='nearest', recompute_scale_factor=True)
        unlabel_region = (scaled_seg_label.long() == 255).squeeze(1)
        return loss_layer.weight * DenseEnergyLossFunction.apply(scaled_images, scaled_segs, loss_layer.sigma_rgb,
                                                                 loss_layer.sigma_xy * sf, scaled_ROIs, unlabel_region)
    pred_prob = F.softmax(logit.float(), dim=1)
    return loss_layer(_img, pred_prob, crop_mask, seg_label)


# --------------------------------------------------------------------------------------------
# seg_refine_by_label / cam_loss  (utils/seg_helper.py:553-568, 593-602)
# --------------------------------------------------------------------------------------------
def seg_refine_by_label(seg, cls_label, softmaxtemp, after_softmax=False):
    b, c, h, w = seg.shape
    cls_label_bk = torch.cat([torch.ones(b, 1, device=cls_label.device, dtype=cls_label.dtype), cls_label], dim=1)
    if after_softmax:
        seg = F.softmax(seg / softmaxtemp, dim=1)
        return cls_label_bk[:, :, None, None] * seg
    valid_seg = torch.where((cls_label_bk == 0)[:, :, None, None], torch.full_like(seg, -1e5), seg)
    return F.softmax(valid_seg / softmaxtemp, dim=1)


def _scale_args(seg_scales):
    """the per-scale low-res teacher segs [2B,K,h_i,w_i] as cosa_cam_loss_targets_m / cosa_cam_label take them -> (ptrs, hs, ws, n, B, K)"""
    n = len(seg_scales)
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in seg_scales])
    hs = _C.int_array([t.shape[2] for t in seg_scales])
    ws = _C.int_array([t.shape[3] for t in seg_scales])
    b2, K = seg_scales[0].shape[:2]
    return ptrs, hs, ws, n, b2 // 2, K


def cam_loss_targets(seg_scales, cls_label, S, out_hw, softmaxtemp, after_softmax=False):
    """seg_refine_by_label(sum_scales seg, T, after_softmax)[:, 1:] bilinearly resized to `out_hw` (main.py:227-228, seg_helper.py:553-568,
    595-597), computed from the per-scale low-res teacher segs without building the [b,K,S,S] tensor."""
    ptrs, hs, ws, n, B, K = _scale_args(seg_scales)
    oh, ow = out_hw
    out = torch.empty((B, K - 1, oh, ow), device=seg_scales[0].device, dtype=torch.float32)
    lab = cls_label.contiguous().float()
    _C.check(_C.lib().cosa_cam_loss_targets_m(ptrs, hs, ws, n, _C.ptr(lab), _C.ptr(out), B, K, int(S), oh, ow, float(softmaxtemp),
                                              int(bool(after_softmax)), _C.stream_ptr()), "cosa_cam_loss_targets_m")
    return out


class _ValueAndGradFn(torch.autograd.Function):
    """a scalar loss whose kernel writes the value and d loss / d x (for a unit upstream gradient) in one call: forward saves the gradient,
    backward scales it.  A subclass gives `launch(x, grad, loss, *rest)`, the kernel call on a contiguous x; `rest` receives no gradient."""

    @classmethod
    def forward(cls, ctx, x, *rest):
        x = x.contiguous()
        grad = torch.empty_like(x)
        loss = torch.empty(1, device=x.device, dtype=torch.float32)
        cls.launch(x, grad, loss, *rest)
        ctx.save_for_backward(grad)
        ctx.n_rest = len(rest)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return (grad * g,) + (None,) * ctx.n_rest


class _MultilabelSoftMarginFn(_ValueAndGradFn):
    """F.multilabel_soft_margin_loss(v, y), v = x or relu(x), value and gradient from one kernel pass (cosa_msm_loss)"""

    @staticmethod
    def launch(x, grad, loss, y, relu):
        y = y.contiguous().float()
        if x.dim() == 4:
            B, C, H, W = x.shape
            R, HW = B * H * W, H * W
        else:
            R, C = x.shape
            HW = 1
        ws = torch.empty((R + 255) // 256, device=x.device, dtype=torch.float64)
        _C.check(_C.lib().cosa_msm_loss(_C.ptr(x), _C.ptr(y), _C.ptr(grad), _C.ptr(loss), _C.ptr(ws), R, C, HW, int(relu), _C.stream_ptr()),
                 "cosa_msm_loss")


def multilabel_soft_margin(x, y, relu=False):
    """F.multilabel_soft_margin_loss(relu(x) if relu else x, y) over the class dimension (dim 1 of [R,C] or [B,C,H,W] logits: every pixel a
    row, as cam_loss flattens them): the fused kernel for fp32 CUDA logits, torch otherwise"""
    if x.is_cuda and x.dtype == torch.float32 and x.dim() in (2, 4) and y.shape == x.shape:
        return _MultilabelSoftMarginFn.apply(x, y, relu)
    v = F.relu(x) if relu else x
    if x.dim() == 4:
        C = x.shape[1]
        v, y = v.float().permute(0, 2, 3, 1).reshape(-1, C), y.permute(0, 2, 3, 1).reshape(-1, C)
    return F.multilabel_soft_margin_loss(v.float(), y)


def cam_loss_from_targets(cam, targets, is_relu=True):
    """cam_loss (seg_helper.py:593-602) given pre-resized targets [B,C,H,W]"""
    if cam.is_cuda and cam.dtype == torch.float32 and targets.shape == cam.shape:
        return multilabel_soft_margin(cam, targets, relu=is_relu)
    B, C, H, W = cam.shape
    if is_relu:
        cam = F.relu(cam)
    cam_flat = cam.float().permute(0, 2, 3, 1).reshape(B * H * W, C)
    tgt_flat = targets.permute(0, 2, 3, 1).reshape(B * H * W, C)
    return F.multilabel_soft_margin_loss(cam_flat, tgt_flat)


def cam_loss(cam, seg_ps, is_relu=True):
    B, C, H, W = cam.shape
    seg_ps_fg = seg_ps[:, 1:, ...]
    seg_ps_fg = F.interpolate(seg_ps_fg, size=[H, W], mode='bilinear', align_corners=False)
    seg_ps_fg_flat = seg_ps_fg.permute(0, 2, 3, 1).reshape(B * H * W, C)
    if is_relu:
        cam = F.relu(cam)
    cam_flat = cam.float().permute(0, 2, 3, 1).reshape(B * H * W, C)
    return F.multilabel_soft_margin_loss(cam_flat, seg_ps_fg_flat)


# --------------------------------------------------------------------------------------------
# cam_lossv2 / cam_lossv3 / cam_lossv3_wrap  (utils/seg_helper.py:604-653, --camloss_version v2 | v3)
# --------------------------------------------------------------------------------------------
CAM_PLANE_MAX = 6400        # h w of one CAM plane the kernels hold in LDS (csrc/loss_kernels.hip: kCamPlaneMax)
CAM_UPSAMPLE_MIN = 8        # the least up-sampling factor of the cross-entropy's LDS tile (csrc/loss_kernels.hip: TC)


def _cam_minmax_norm(cam, detach=False):
    """(relu(cam) - min) / (max + 1e-4) per plane; the extrema through adaptive_max_pool2d, which routes the gradient to the first position
    of each (a plain amin / amax would spread it over ties)"""
    r = F.relu(cam.float())
    lo, hi = F.adaptive_max_pool2d(-r, (1, 1)), F.adaptive_max_pool2d(r, (1, 1)) + 1e-4
    if detach:
        lo, hi = lo.detach(), hi.detach()
    return (r + lo) / hi


def _cam_lossv2_torch(cam, targets, detach=False):
    """cam_lossv2 given targets at the CAM's size, op by op: the composition the kernels are checked against (fused_losses=False, host
    tensors, detach=True, shapes outside the kernels' envelope)"""
    B, C, H, W = cam.shape
    n = _cam_minmax_norm(cam, detach)
    return F.multilabel_soft_margin_loss(n.permute(0, 2, 3, 1).reshape(B * H * W, C), targets.permute(0, 2, 3, 1).reshape(B * H * W, C))


def _cam_lossv3_torch(cam, seg_label, detach=False, cambgmax=True):
    """cam_lossv3 op by op (see _cam_lossv2_torch): the class-balanced cross-entropy of the up-sampled [background, n] planes"""
    n = _cam_minmax_norm(cam, detach)
    bg = 1 - (torch.max(n, dim=1, keepdim=True)[0] if cambgmax else torch.mean(n, dim=1, keepdim=True))
    mix = F.interpolate(torch.cat([bg, n], dim=1), size=list(seg_label.shape[-2:]), mode='bilinear', align_corners=False)
    return seg_loss(mix, seg_label)


def _cam_label_torch(seg_ps, seg_confident_thre):
    """cam_lossv3_wrap's label map: the class of the largest probability (lowest index at a tie), 255 where it is not above the threshold"""
    value, label = torch.max(seg_ps, dim=1)
    return torch.where(value <= seg_confident_thre, torch.full_like(label, 255), label)


def _cam_kernel_ok(cam, S=None):
    """fp32 device CAMs inside the plane kernels' envelope (and, for v3, a label map the cross-entropy's tile can serve)"""
    if not (cam.is_cuda and cam.dtype == torch.float32 and cam.dim() == 4):
        return False
    B, C, h, w = cam.shape
    if not (0 < B <= 65535 and 0 < C < 128 and 0 < h * w <= CAM_PLANE_MAX):
        return False
    return S is None or (S[0] == S[1] and S[0] % 2 == 0 and S[0] >= CAM_UPSAMPLE_MIN * h and S[0] >= CAM_UPSAMPLE_MIN * w)


class _CamLossV2Fn(_ValueAndGradFn):
    """cam_lossv2 on targets at the CAM's size, value and gradient from one launch per plane (cosa_cam_lossv2)"""

    @staticmethod
    def launch(cam, grad, loss, targets):
        targets = targets.contiguous().float()
        B, C, h, w = cam.shape
        L = _C.lib()
        ws = _C.workspace(L.cosa_cam_lossv2_workspace_bytes(B, C), cam.device, "cam_lossv2")
        _C.check(L.cosa_cam_lossv2(_C.ptr(cam), _C.ptr(targets), _C.ptr(grad), _C.ptr(loss), B, C, h, w, _C.ptr(ws), ws.numel(), _C.stream_ptr()),
                 "cosa_cam_lossv2")


class _CamLossV3Fn(_ValueAndGradFn):
    """cam_lossv3 against a byte label map [B,S,S], value and gradient from one call (cosa_cam_lossv3); nothing of size [B,K,S,S] is written"""

    @staticmethod
    def launch(cam, grad, loss, label):
        B, C, h, w = cam.shape
        L = _C.lib()
        ws = _C.workspace(L.cosa_cam_lossv3_workspace_bytes(B, C, h, w), cam.device, "cam_lossv3")
        _C.check(L.cosa_cam_lossv3(_C.ptr(cam), _C.ptr(label), _C.ptr(grad), _C.ptr(loss), B, C, h, w, label.shape[-1], _C.ptr(ws), ws.numel(),
                                   _C.stream_ptr()), "cosa_cam_lossv3")


def cam_lossv2_from_targets(cam, targets):
    """cam_lossv2 (seg_helper.py:604-624) given pre-resized targets [B,C,H,W] (cam_loss_targets): the fused kernel for fp32 device CAMs
    inside its envelope, the torch composition otherwise"""
    if _cam_kernel_ok(cam) and targets.is_cuda and targets.shape == cam.shape:
        return _CamLossV2Fn.apply(cam, targets)
    return _cam_lossv2_torch(cam, targets)


def cam_lossv2(cam, seg_ps, detach=False):
    B, C, H, W = cam.shape
    targets = F.interpolate(seg_ps[:, 1:, ...], size=[H, W], mode='bilinear', align_corners=False)
    if detach:
        return _cam_lossv2_torch(cam, targets, detach=True)
    return cam_lossv2_from_targets(cam, targets)


def cam_lossv3(cam, seg_label, detach=False, cambgmax=True):
    """seg_label [B,H,W]: 0 background, 1..C, 255 ignored (any integer dtype, or the bytes cam_label_from_scales writes)"""
    if not detach and cambgmax and seg_label.is_cuda and seg_label.dim() == 3 and _cam_kernel_ok(cam, tuple(seg_label.shape[-2:])) \
            and seg_label.shape[0] == cam.shape[0]:
        lab = seg_label if seg_label.dtype == torch.uint8 else seg_label.to(torch.uint8)
        return _CamLossV3Fn.apply(cam, lab.contiguous())
    return _cam_lossv3_torch(cam, seg_label, detach=detach, cambgmax=cambgmax)


def cam_lossv3_wrap(cam, seg_ps, seg_confident_thre=0.25):
    return cam_lossv3(cam, _cam_label_torch(seg_ps, seg_confident_thre))


def cam_label_from_scales(seg_scales, cls_label, S, softmaxtemp, segconf_thre, after_softmax=False):
    """cam_lossv3_wrap's label map, bytes [B,S,S], from the per-scale low-res teacher segs (cam_loss_targets' inputs) without building the
    [b,K,S,S] tensor: argmax of seg_refine_by_label(sum_scales seg, T, after_softmax), 255 where its maximum is not above segconf_thre"""
    ptrs, hs, ws, n, B, K = _scale_args(seg_scales)
    out = torch.empty((B, int(S), int(S)), device=seg_scales[0].device, dtype=torch.uint8)
    lab = cls_label.contiguous().float()
    _C.check(_C.lib().cosa_cam_label(ptrs, hs, ws, n, _C.ptr(lab), _C.ptr(out), B, K, int(S), float(softmaxtemp), float(segconf_thre),
                                     int(bool(after_softmax)), _C.stream_ptr()), "cosa_cam_label")
    return out


# --------------------------------------------------------------------------------------------
# the supervised-contrastive token loss: this project's own objective, not the reference's
# --------------------------------------------------------------------------------------------
TOKCON_DIM = 768            # the kernels' envelope (csrc/tokcon_kernels.hip): bf16 device tokens of this width ...
TOKCON_MAX_N = 4096         # ... 2 <= n <= this many per image ...
TOKCON_TEMP = (0.01, 10.0)  # ... and a temperature in this range
TOKCON_IGNORE = 255


def check_tokcon_settings(weight, temp, purity, flag=""):
    """the term's three settings (trainer: flag "", launcher: flag "--"), or a ValueError naming the one outside its range"""
    if not (math.isfinite(float(weight)) and float(weight) >= 0):
        raise ValueError(f"{flag}tokcon_weight {weight!r}: 0 (off) or a positive weight")
    if not TOKCON_TEMP[0] <= float(temp) <= TOKCON_TEMP[1]:
        raise ValueError(f"{flag}tokcon_temp {temp!r}: a temperature in [{TOKCON_TEMP[0]}, {TOKCON_TEMP[1]}]")
    if not 0.5 < float(purity) <= 1.0:
        raise ValueError(f"{flag}tokcon_purity {purity!r}: a share of the cell's pixels in (0.5, 1]")


def token_need(patch, purity=1.0):
    """ceil(purity * patch^2) as an integer: the pixels of a cell one class must hold for the token to take its label"""
    if not 0.5 < float(purity) <= 1.0:
        raise ValueError(f"purity {purity!r}: a share of the cell's pixels in (0.5, 1]")
    pp = int(patch) * int(patch)
    return min(max(int(math.ceil(float(purity) * pp)), pp // 2 + 1), pp)          # (the clamp: a no-op for a purity in range)


def _token_labels_torch(mask, patch, need):
    B, S = mask.shape[0], mask.shape[-1]
    g = S // patch
    cells = mask.reshape(B, g, patch, g, patch).permute(0, 1, 3, 2, 4).reshape(B, g * g, patch * patch).long()
    mode = cells.mode(dim=-1).values
    cnt = (cells == mode.unsqueeze(-1)).sum(-1)
    return torch.where((cnt >= need) & (mode != TOKCON_IGNORE), mode, torch.full_like(mode, TOKCON_IGNORE)).to(torch.uint8)


def token_labels(mask, patch, purity=1.0):
    """label map [B,S,S] (any integer dtype, values 0..255, 255 = ignore) -> uint8 [B,(S/patch)^2]: token (r, c) takes the class that holds at
    least ceil(purity * patch^2) of the pixels of its cell, 255 when none does (background is a class like any other).  One kernel of
    byte loads and integer counts for device maps (cosa_token_labels), torch for host maps."""
    patch = int(patch)
    if mask.dim() != 3 or mask.shape[1] != mask.shape[2] or patch < 1 or mask.shape[-1] % patch != 0:
        raise ValueError(f"token_labels: a square label map [B,S,S] whose side the patch size divides (got {tuple(mask.shape)}, patch {patch})")
    need = token_need(patch, purity)
    if not mask.is_cuda:
        return _token_labels_torch(mask, patch, need)
    if mask.dtype not in (torch.uint8, torch.int64):
        mask = mask.to(torch.int64)
    mask = mask.contiguous()
    B, S = mask.shape[0], mask.shape[-1]
    out = torch.empty((B, (S // patch) ** 2), device=mask.device, dtype=torch.uint8)
    _C.check(_C.lib().cosa_token_labels(_C.ptr(mask), mask.element_size(), _C.ptr(out), B, S, patch, need, _C.stream_ptr()), "cosa_token_labels")
    return out


def _token_contrast_torch(tokens, labels, temp, return_count=False):
    """the term op by op in torch (float32 for 16-bit tokens, else the tokens' own dtype): what the kernels are checked against, and the path
    of host tensors, other dtypes, shapes outside the envelope and fused_losses=False.  -> loss, or (loss, M) with return_count"""
    x = tokens.float() if tokens.dtype in (torch.bfloat16, torch.float16) else tokens
    y = labels.long()
    n = x.shape[1]
    z = x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    s = torch.matmul(z, z.transpose(1, 2)) / temp
    valid = y != TOKCON_IGNORE
    off = ~torch.eye(n, dtype=torch.bool, device=x.device)
    A = valid.unsqueeze(1) & off                                              # [B, i, j]: j in A(i)
    P = A & valid.unsqueeze(2) & (y.unsqueeze(2) == y.unsqueeze(1))
    npos = P.sum(-1)
    anchor = npos >= 1
    # (only anchor rows are masked: a row of -inf alone would put NaN into the backward of the rows torch.where drops)
    lse = torch.logsumexp(s.masked_fill(~A & anchor.unsqueeze(2), float("-inf")), dim=-1)
    pos = (s * P.to(s.dtype)).sum(-1) / npos.clamp_min(1).to(s.dtype)
    M = anchor.sum()
    loss = torch.where(anchor, lse - pos, torch.zeros_like(lse)).sum() / M.clamp_min(1).to(s.dtype)
    return (loss, M) if return_count else loss


def _tokcon_kernel_ok(tokens, labels, temp):
    return (tokens.is_cuda and labels.is_cuda and tokens.dtype == torch.bfloat16 and tokens.dim() == 3 and tokens.shape[2] == TOKCON_DIM
            and 2 <= tokens.shape[1] <= TOKCON_MAX_N and 1 <= tokens.shape[0] <= 65535 and TOKCON_TEMP[0] <= float(temp) <= TOKCON_TEMP[1])


class _TokenContrastFn(Function):
    """value and saved statistics (per-token log-sum-exp and positive sum, per-image class counts, M) from one forward call
    (cosa_token_contrast_fwd), the bf16 gradient from one backward call (cosa_token_contrast_bwd)"""

    @staticmethod
    def forward(ctx, tokens, labels, temp):
        B, n, D = tokens.shape
        L = _C.lib()
        rows = torch.empty((2, B, n), device=tokens.device, dtype=torch.float32)
        counts = torch.empty(B * 256 + 1, device=tokens.device, dtype=torch.int32)
        loss = torch.empty(1, device=tokens.device, dtype=torch.float32)
        ws = _C.workspace(L.cosa_token_contrast_workspace_bytes(B, n), tokens.device, "token_contrast")
        _C.check(L.cosa_token_contrast_fwd(_C.ptr(tokens), _C.ptr(labels), _C.ptr(rows), _C.ptr(counts), _C.ptr(loss), B, n, D, float(temp),
                                           _C.ptr(ws), ws.numel(), _C.stream_ptr()), "cosa_token_contrast_fwd")
        ctx.save_for_backward(tokens, labels, rows, counts)
        ctx.temp = float(temp)
        ctx.mark_non_differentiable(counts)
        return loss[0], counts

    @staticmethod
    def backward(ctx, g, _g_counts):
        tokens, labels, rows, counts = ctx.saved_tensors
        B, n, D = tokens.shape
        L = _C.lib()
        up = g.detach().reshape(1).float().contiguous()
        dx = torch.empty_like(tokens)
        ws = _C.workspace(L.cosa_token_contrast_workspace_bytes(B, n), tokens.device, "token_contrast")
        _C.check(L.cosa_token_contrast_bwd(_C.ptr(tokens), _C.ptr(labels), _C.ptr(rows), _C.ptr(counts), _C.ptr(up), _C.ptr(dx), B, n, D,
                                           ctx.temp, _C.ptr(ws), ws.numel(), _C.stream_ptr()), "cosa_token_contrast_bwd")
        return dx, None, None


def token_contrast_loss(tokens, labels, temp, return_count=False):
    """The supervised-contrastive token loss (the form of Khosla et al. 2020) of tokens [B,n,D] under token labels [B,n] (255 = unlabelled),
    each image on its own: with z_i = x_i / max(|x_i|, 1e-12), s_ij = z_i . z_j / temp, A(i) the labelled j != i, P(i) those of i's label,
    anchors the labelled i with |P(i)| >= 1 and M their number over the batch,
        L = (1/M) sum_anchors (log sum_{A(i)} exp s_ia - (1/|P(i)|) sum_{P(i)} s_ij);   M = 0: L = 0 exactly and a zero gradient.
    Both sides of every pair carry gradient.  bf16 device tokens of width 768 with 2 <= n <= 4096 and 0.01 <= temp <= 10 run on the HIP kernels
    (csrc/tokcon_kernels.hip), anything else on the torch composition.  -> loss (fp32 scalar), or (loss, M) with return_count; no host sync."""
    if labels.shape != tokens.shape[:2]:
        raise ValueError(f"token_contrast_loss: labels {tuple(labels.shape)} for tokens {tuple(tokens.shape)}")
    if _tokcon_kernel_ok(tokens, labels, temp):
        lab = labels if labels.dtype == torch.uint8 else labels.to(torch.uint8)
        loss, counts = _TokenContrastFn.apply(tokens.contiguous(), lab.contiguous(), float(temp))
        return (loss, counts[-1]) if return_count else loss
    return _token_contrast_torch(tokens, labels, temp, return_count=return_count)


# --------------------------------------------------------------------------------------------
# the reliability-weighted seg loss: the reference's seg_weightloss (utils/seg_helper.py:823-835, called by nothing
# there) under this project's own weight -- how far the CAM behind a pseudo label lies from the threshold it passed
# --------------------------------------------------------------------------------------------
RELIABILITY_BETA = (0.0, 8.0)      # --camweight_beta: the exponent on the distance, in [0, 8]; 0: every labelled pixel weighs 1
RELIABILITY_MAX_SETS = 4           # the kernel's envelope (csrc/reliability_kernels.hip): CAM sets per launch ...
RELIABILITY_MAX_C = 255            # ... and classes
_REL_FIX = 4294967296.0            # the counters' fixed point: rint(w * 2^32)


def check_reliability_settings(beta, floor, flag=""):
    """the weight's two settings (trainer: flag "", launcher: flag "--"), or a ValueError naming the one outside its range"""
    if not RELIABILITY_BETA[0] <= float(beta) <= RELIABILITY_BETA[1]:
        raise ValueError(f"{flag}camweight_beta {beta!r}: an exponent in [{RELIABILITY_BETA[0]:g}, {RELIABILITY_BETA[1]:g}]")
    if not 0.0 <= float(floor) < 1.0:
        raise ValueError(f"{flag}seg_reliability_floor {floor!r}: the weight of a pixel the CAM does not support, in [0, 1)")


def new_reliability_stats(G, device):
    """zeroed counters int64 [G][4] = {Sum_bg rint(w 2^32), n_bg, Sum_fg rint(w 2^32), n_fg} per CAM set"""
    return torch.zeros((int(G), 4), device=device, dtype=torch.int64)


def _reliability_shapes(cams_list, cls_labels, masks, thresholds_high, thresholds_low, stats):
    G = len(cams_list)
    if not (1 <= G <= RELIABILITY_MAX_SETS and len(masks) == G and len(thresholds_high) == G and len(thresholds_low) == G):
        raise ValueError(f"label_reliability: 1 to {RELIABILITY_MAX_SETS} CAM sets, each with its label map and (high, low) threshold pair")
    b, C, h, w = cams_list[0].shape
    if h != w or not 1 <= C <= RELIABILITY_MAX_C or cls_labels.shape != (b, C):
        raise ValueError(f"label_reliability: cams [b,C,S,S] with 1 <= C <= {RELIABILITY_MAX_C} and cls_labels [b,C] "
                         f"(got {tuple(cams_list[0].shape)}, {tuple(cls_labels.shape)})")
    for c, m in zip(cams_list, masks):
        if c.shape != (b, C, h, w) or m.shape != (b, h, w):
            raise ValueError("label_reliability: every CAM set [b,C,S,S] with a label map [b,S,S]")
    if stats is not None and (stats.shape != (G, 4) or stats.dtype != torch.int64 or not stats.is_contiguous()
                              or stats.device != cams_list[0].device):
        raise ValueError(f"label_reliability: stats must be contiguous int64 [{G}][4] on the CAMs' device (new_reliability_stats)")
    return G, b, C, h


def _label_reliability_torch(cams_list, cls_labels, masks, thresholds_high, thresholds_low, beta=1.0, floor=0.0, stats=None):
    """label_reliability op by op in fp32 torch, in the kernel's operation order: what the kernel is checked against, and the path of host
    tensors and of fused_losses=False"""
    check_reliability_settings(beta, floor)
    G, b, C, S = _reliability_shapes(cams_list, cls_labels, masks, thresholds_high, thresholds_low, stats)
    dev = cams_list[0].device
    f32 = lambda v: torch.as_tensor(v, device=dev).reshape(()).to(torch.float32)
    beta, floor = float(np.float32(beta)), float(np.float32(floor))
    omf = float(np.float32(1.0) - np.float32(floor))
    y = cls_labels.to(torch.float32)
    out = []
    for g in range(G):
        hi, lo = f32(thresholds_high[g]), f32(thresholds_low[g])
        cam = cams_list[g].to(torch.float32) * y[:, :, None, None]
        l = masks[g].to(torch.float32).to(torch.int64)
        bg, fg = l == 0, (l >= 1) & (l <= C)
        m = cam.amax(dim=1)
        v = cam.gather(1, (l - 1).clamp(0, C - 1).unsqueeze(1)).squeeze(1)
        r = torch.where(bg, (lo - m) / lo, (v - hi) / (1.0 - hi))
        r = torch.where(r != r, torch.zeros_like(r), r.clamp(0.0, 1.0))
        if beta == 0.0:
            u = torch.ones_like(r)
        elif beta == 1.0:
            u = r
        else:
            u = torch.where(r == 0, torch.zeros_like(r), torch.exp2(beta * torch.log2(r)))
        w = torch.where(bg | fg, floor + omf * u, torch.zeros_like(u))
        if stats is not None:
            q = torch.round(w.double() * _REL_FIX).to(torch.int64)
            stats[g] += torch.stack([(q * bg).sum(), bg.sum(), (q * fg).sum(), fg.sum()])
        out.append(w)
    return out


def label_reliability(cams_list, cls_labels, masks, thresholds_high, thresholds_low, beta=1.0, floor=0.0, stats=None):
    """One weight map [b,S,S] fp32 in [0, 1] per CAM set: how far the CAM behind each pseudo label lies from the threshold it passed.
    For set g with thresholds (hi, lo) -- floats or device scalars --, label l = masks[g][b,p] and class row y = cls_labels[b], all fp32:
        l == 0:       m = max_c (y[c] cam[b,c,p]),  r = (lo - m) / lo          (background: how far every present class stays below `lo`)
        1 <= l <= C:  v = y[l-1] cam[b,l-1,p],      r = (v - hi) / (1 - hi)    (foreground: how far its own class rises above `hi`)
        otherwise:    w = 0
        r = 0 where it is NaN, else clamped to [0, 1];  u = r ** beta (beta 0: 1, beta 1: r itself);  w = floor + (1 - floor) u
    Multiplying by y folds cam_validation in and is idempotent: raw and validated CAMs give the same map.  hi == lo makes it the distance
    from one threshold; beta = 0 weighs every labelled pixel 1.  A label the CAM does not support -- PAR moved it there, or its class is
    absent from y -- has r = 0 and weighs `floor`.
    `stats` (new_reliability_stats(G)): counters the call ADDS to (reliability_summary reads them).
    Device tensors: one launch for all sets (cosa_label_reliability), no host sync, device thresholds read on the device.  Host tensors:
    the torch composition (_label_reliability_torch)."""
    check_reliability_settings(beta, floor)
    if not cams_list[0].is_cuda:
        return _label_reliability_torch(cams_list, cls_labels, masks, thresholds_high, thresholds_low, beta, floor, stats)
    _C.require_cuda(cls_labels, *cams_list, *masks)
    G, b, C, S = _reliability_shapes(cams_list, cls_labels, masks, thresholds_high, thresholds_low, stats)
    dev = cams_list[0].device
    cams_list = [c.contiguous().float() for c in cams_list]
    masks = [m.contiguous().float() for m in masks]
    cls_labels = cls_labels.contiguous().float()
    rel = [torch.empty((b, S, S), device=dev, dtype=torch.float32) for _ in range(G)]
    ptrs = lambda ts: (ctypes.c_void_p * G)(*[t.data_ptr() for t in ts])
    if any(torch.is_tensor(t) for t in list(thresholds_high) + list(thresholds_low)):
        # thresholds that live on the device (adaptive thresholds): [G][hi, lo] float32, read by the kernel -- no host sync
        tdev = torch.stack([torch.stack([torch.as_tensor(h, device=dev).reshape(()).to(torch.float32),
                                         torch.as_tensor(l, device=dev).reshape(()).to(torch.float32)])
                            for h, l in zip(thresholds_high, thresholds_low)]).contiguous()
        hi = lo = (ctypes.c_float * G)(*([0.0] * G))
    else:
        tdev = None
        hi = (ctypes.c_float * G)(*[float(t) for t in thresholds_high])
        lo = (ctypes.c_float * G)(*[float(t) for t in thresholds_low])
    _C.check(_C.lib().cosa_label_reliability(ptrs(cams_list), _C.ptr(cls_labels), ptrs(masks), ptrs(rel), hi, lo, _C.ptr(tdev), G, b, C, S,
                                             float(beta), float(floor), _C.ptr(stats), _C.stream_ptr()), "cosa_label_reliability")
    return rel


def reliability_summary(stats):
    """counters [G][4] (label_reliability's `stats`) -> one dict per CAM set: the mean weight of its background and of its foreground pixels
    (None for a group without a pixel) and the two pixel counts.  Synchronises."""
    rows = stats.tolist()
    mean = lambda s, n: (s / _REL_FIX / n) if n else None
    return [dict(bg=mean(r[0], r[1]), n_bg=r[1], fg=mean(r[2], r[3]), n_fg=r[3]) for r in rows]


def seg_weightloss(seg_pred, mask_label, mask_weights, fg_alpha=0.5, ignore_index=255):
    """utils/seg_helper.py:823-835: seg_loss with every pixel's cross-entropy multiplied by `mask_weights` [b,h,w]; the denominators stay the
    plain counts of labelled pixels.  One log-softmax pass shared by the two class-balanced terms, as seg_loss."""
    assert fg_alpha >= 0 and fg_alpha <= 1, "fg_alpha should be in [0,1]"
    lab = mask_label.long()
    bg_label = torch.where(lab != 0, torch.full_like(lab, ignore_index), lab)
    fg_label = torch.where(lab == 0, torch.full_like(lab, ignore_index), lab)
    logp = F.log_softmax(seg_pred.float(), dim=1)
    bg_loss_raw = F.nll_loss(logp, bg_label, ignore_index=ignore_index, reduction='none')
    bg_loss = (bg_loss_raw * mask_weights).sum() / ((bg_label != ignore_index).sum() + 1e-6)
    fg_loss_raw = F.nll_loss(logp, fg_label, ignore_index=ignore_index, reduction='none')
    fg_loss = (fg_loss_raw * mask_weights).sum() / ((fg_label != ignore_index).sum() + 1e-6)
    return (1 - fg_alpha) * bg_loss + fg_alpha * fg_loss


# --------------------------------------------------------------------------------------------
# the soft-label seg loss distilled from the teacher's segmentation: the reference's seg_softloss / seg_softlossv2
# (utils/seg_helper.py:837-861, called by nothing there) against a target this build makes from the teacher's own seg passes
# --------------------------------------------------------------------------------------------
SEG_SOFT_TEMP = (0.05, 20.0)       # --seg_soft_temp: on the MEAN of the teacher's passes
SEG_SOFT_MAX_K = 128               # the kernels' envelope (csrc/loss_kernels.hip: seg_soft_check): classes, background included ...
SEG_SOFT_MAX_SCALES = 4            # ... and teacher scales; the student's logits need the seg-loss tile's factor (CAM_UPSAMPLE_MIN)


def check_seg_soft_settings(weight, temp, conf, flag=""):
    """the term's three settings (trainer: flag "", launcher: flag "--"), or a ValueError naming the one outside its range"""
    if not (math.isfinite(float(weight)) and float(weight) >= 0):
        raise ValueError(f"{flag}seg_soft_weight {weight!r}: 0 (off) or a positive weight")
    if not SEG_SOFT_TEMP[0] <= float(temp) <= SEG_SOFT_TEMP[1]:
        raise ValueError(f"{flag}seg_soft_temp {temp!r}: a temperature in [{SEG_SOFT_TEMP[0]}, {SEG_SOFT_TEMP[1]}]")
    if not 0.0 <= float(conf) < 1.0:
        raise ValueError(f"{flag}seg_soft_conf {conf!r}: a probability in [0, 1); 0: no gate")


def seg_softlossv2(seg_pred, softprobs):
    """utils/seg_helper.py:854-861: - sum_k softprobs_k log_softmax(seg_pred)_k, averaged over the pixels ([B,K,H,W] or rows [N,K]).  The
    reference takes `.mean()`, which is NaN for no pixel at all; here the sum is divided by (count + 1e-6), seg_loss's denominator: no pixel
    gives 0 with a zero gradient, and a mean over n pixels moves by 1e-6 / n of itself."""
    per = -(F.log_softmax(seg_pred, dim=1) * softprobs).sum(dim=1)
    return per.sum() / (per.numel() + 1e-6)


def _seg_soft_torch(seg_pred, softprobs, fg_alpha=0.5, img_box=None, conf=None):
    """the term op by op on full-resolution logits and targets [B,K,H,W]: what the kernels are checked against, and the path of
    fused_losses=False, host tensors and shapes outside the envelope.  A pixel is background where the first argmax of its target is 0 and
    foreground otherwise; outside its box (img_box given) or with max q <= conf (conf given) it is in neither set.  An empty set contributes 0."""
    assert fg_alpha >= 0 and fg_alpha <= 1, "fg_alpha should be in [0,1]"
    value, label = torch.max(softprobs, dim=1)                  # (the lowest index at a tie, as _cam_label_torch)
    keep = torch.ones_like(label, dtype=torch.bool) if conf is None else ~(value <= conf)
    if img_box is not None:
        b, _, h, w = seg_pred.shape
        keep = keep & (_crop_mask_from_boxes(_abs_boxes(img_box, h, w), b, h, w, seg_pred.device) > 0)
    per = -(F.log_softmax(seg_pred, dim=1) * softprobs).sum(dim=1)
    zero = torch.zeros_like(per)
    bg, fg = keep & (label == 0), keep & (label != 0)
    bgloss = torch.where(bg, per, zero).sum() / (bg.sum().to(per.dtype) + 1e-6)       # (the count in the loss's own dtype: 1e-6 survives in float64)
    fgloss = torch.where(fg, per, zero).sum() / (fg.sum().to(per.dtype) + 1e-6)
    return (1 - fg_alpha) * bgloss + fg_alpha * fgloss


def seg_softloss(seg_pred, softprobs, fg_alpha=0.5):
    """utils/seg_helper.py:837-852: seg_softlossv2 over the pixels whose target's argmax is the background and over the others, blended by
    fg_alpha.  The reference's `.mean()` over an empty set is NaN; here each set's sum is divided by (count + 1e-6), so an empty set
    contributes 0 and a zero gradient (seg_softlossv2)."""
    return _seg_soft_torch(seg_pred, softprobs, fg_alpha=fg_alpha)


def _wide(t):
    """float32 for a 16-bit tensor, any other dtype as it is (the torch compositions run in their inputs' precision: float64 in the tests)"""
    return t.float() if t.dtype in (torch.bfloat16, torch.float16) else t


def _abs_boxes(img_box, h, w):
    """boxes (y0, y1, x0, x1) with the reference's slicing semantics (a negative bound counts from the end, cam2mask_multi) in absolute form"""
    if not torch.is_tensor(img_box):
        img_box = torch.as_tensor(img_box)
    size = torch.tensor([h, h, w, w], device=img_box.device, dtype=img_box.dtype)
    return torch.where(img_box < 0, img_box + size, img_box)


def seg_soft_targets_torch(seg, cls_label, S, temp, n_scales=None):
    """the soft target op by op -> q [B,K,S,S].  seg: the list of per-scale low-res teacher segs [2B,K,h_i,w_i] (original batch, then the
    flipped one: multi_scale_camseg's `_seg_scales`), summed here as multi_scale_camseg sums them, or that sum itself [B,K,S,S] (seg_ps)
    with n_scales, the number of scales it holds.  q = softmax(z / (2 n_scales temp)) over the background and the classes of cls_label,
    0 exactly for an absent class."""
    if isinstance(seg, (list, tuple)):
        n, B = len(seg), seg[0].shape[0] // 2
        z = None
        for s in seg:
            up = F.interpolate(s, size=(int(S), int(S)), mode="bilinear", align_corners=False)
            v = up[:B] + up[B:].flip(-1)
            z = v if z is None else z + v
    else:
        if n_scales is None:
            raise ValueError("seg_soft_targets_torch: a summed seg_ps needs n_scales, the number of scales it holds")
        n, z = int(n_scales), seg
    z = z / (2.0 * n * float(temp))
    present = torch.cat([torch.ones_like(cls_label[:, :1]), cls_label], dim=1) != 0
    z = torch.where(present[:, :, None, None], z, torch.full_like(z, float("-inf")))
    return F.softmax(z, dim=1)


def seg_soft_loss_torch(seg_up, seg, cls_label, img_box, temp, conf, fg_alpha, n_scales=None):
    """the term on the student's up-sampled logits seg_up [B,K,S,S] by the torch composition (seg, n_scales: seg_soft_targets_torch's)"""
    with torch.no_grad():
        q = seg_soft_targets_torch(seg, cls_label, seg_up.shape[-1], temp, n_scales=n_scales)
    return _seg_soft_torch(_wide(seg_up), q, fg_alpha=fg_alpha, img_box=img_box, conf=conf)


def _seg_soft_kernel_ok(seg_lr, seg_scales, cls_label, S):
    if not (isinstance(seg_scales, (list, tuple)) and 1 <= len(seg_scales) <= SEG_SOFT_MAX_SCALES):
        return False
    if not (seg_lr.is_cuda and seg_lr.dtype == torch.float32 and seg_lr.dim() == 4 and cls_label.is_cuda):
        return False
    B, K, h, w = seg_lr.shape
    if not (0 < B <= 65535 and 2 <= K <= SEG_SOFT_MAX_K and S % 2 == 0 and S >= CAM_UPSAMPLE_MIN * h and S >= CAM_UPSAMPLE_MIN * w):
        return False
    return all(t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.shape[0] == 2 * B and t.shape[1] == K and
               0 < t.shape[2] <= S and 0 < t.shape[3] <= S for t in seg_scales) and tuple(cls_label.shape) == (B, K - 1)


class _SegSoftFn(Function):
    """the value and the four sums from one forward launch (cosa_seg_soft_forward); the gradient of the student's low-res logits from one
    backward launch that reads those sums on the device (cosa_seg_soft_backward).  The target is a constant: no other input has a gradient."""

    @staticmethod
    def forward(ctx, seg_lr, labels, boxes, S, temp, conf, fg_alpha, *seg_scales):
        B, K, h, w = seg_lr.shape
        L = _C.lib()
        ptrs, hs, ws, n, _, _ = _scale_args(seg_scales)
        sums = torch.empty(4, device=seg_lr.device, dtype=torch.float32)
        loss = torch.empty(1, device=seg_lr.device, dtype=torch.float32)
        wsp = _C.workspace(L.cosa_seg_soft_workspace_bytes(B, K, h, w), seg_lr.device, "seg_soft")
        _C.check(L.cosa_seg_soft_forward(_C.ptr(seg_lr), ptrs, hs, ws, n, _C.ptr(labels), _C.ptr(boxes), _C.ptr(sums), _C.ptr(loss), B, K, h, w,
                                         int(S), float(temp), float(conf), float(fg_alpha), _C.ptr(wsp), wsp.numel(), _C.stream_ptr()),
                 "cosa_seg_soft_forward")
        ctx.save_for_backward(seg_lr, labels, boxes, sums, *seg_scales)
        ctx.cfg = (int(S), float(temp), float(conf), float(fg_alpha))
        ctx.mark_non_differentiable(sums)
        return loss[0], sums

    @staticmethod
    def backward(ctx, g, _g_sums):
        seg_lr, labels, boxes, sums, *seg_scales = ctx.saved_tensors
        S, temp, conf, fg_alpha = ctx.cfg
        B, K, h, w = seg_lr.shape
        L = _C.lib()
        ptrs, hs, ws, n, _, _ = _scale_args(seg_scales)
        up = g.detach().reshape(1).float().contiguous()
        grad = torch.empty_like(seg_lr)
        wsp = _C.workspace(L.cosa_seg_soft_workspace_bytes(B, K, h, w), seg_lr.device, "seg_soft")
        _C.check(L.cosa_seg_soft_backward(_C.ptr(seg_lr), ptrs, hs, ws, n, _C.ptr(labels), _C.ptr(boxes), _C.ptr(sums), _C.ptr(up), _C.ptr(grad),
                                          B, K, h, w, S, temp, conf, fg_alpha, _C.ptr(wsp), wsp.numel(), _C.stream_ptr()),
                 "cosa_seg_soft_backward")
        return (grad,) + (None,) * (6 + len(seg_scales))


def seg_soft_loss(seg_lr, seg_scales, cls_label, img_box, S, temp=1.0, conf=0.0, fg_alpha=0.5, return_sums=False):
    """The soft-label seg loss of the student's low-res logits seg_lr [B,K,h,w] against the teacher's per-scale low-res
    segs seg_scales (list of [2B,K,h_i,w_i]: original batch, then the flipped one).  Per full-resolution pixel inside its box img_box[b] =
    (y0, y1, x0, x1): z = the sum of the up-sampled passes (multi_scale_camseg's sum), q = softmax(z / (2 n_scales temp)) over the background
    and the classes of cls_label (0 exactly for an absent class), l = - sum_k q_k log softmax(up(seg_lr))_k; background set: the first argmax of
    q is 0, foreground set: it is not; neither where max q <= conf;
        L = (1 - fg_alpha) sum_bg l / (n_bg + 1e-6) + fg_alpha sum_fg l / (n_fg + 1e-6)     (an empty set contributes 0).
    The gradient goes to seg_lr only.  fp32 device tensors inside the kernels' envelope (K <= 128, at most 4 scales of at most S x S, S even
    and >= 8 h) run on the HIP kernels, which write nothing of size [B,K,S,S]; anything else takes the torch composition.
    -> loss (fp32 scalar), or (loss, sums = [sum_bg, n_bg, sum_fg, n_fg]) with return_sums (kernels only; None on the torch path)."""
    check_seg_soft_settings(0.0, temp, conf)
    S = int(S)
    if _seg_soft_kernel_ok(seg_lr, seg_scales, cls_label, S):
        boxes = _boxes_to_device(_abs_boxes(img_box, S, S), seg_lr.device)
        if tuple(boxes.shape) != (seg_lr.shape[0], 4):
            raise ValueError("seg_soft_loss: img_box must be [b,4]")
        loss, sums = _SegSoftFn.apply(seg_lr.contiguous(), cls_label.contiguous().float(), boxes, S, float(temp), float(conf), float(fg_alpha),
                                      *[t.contiguous() for t in seg_scales])
        return (loss, sums) if return_sums else loss
    up = F.interpolate(_wide(seg_lr), size=(S, S), mode="bilinear", align_corners=False)
    loss = seg_soft_loss_torch(up, seg_scales, cls_label, img_box, temp, conf, fg_alpha)
    return (loss, None) if return_sums else loss


# --------------------------------------------------------------------------------------------
# dense-CRF post-processing of the final evaluation  (utils/seg_helper.py:961-996)
# --------------------------------------------------------------------------------------------
class DenseCRF(object):
    """utils/seg_helper.py:961-987, same constructor and call: `DenseCRF(...)(image [H,W,3] uint8, probmap [C,H,W])` -> Q [C,H,W].

    The reference delegates to pydensecrf (DenseCRF2D: setUnaryEnergy(-log p), addPairwiseGaussian, addPairwiseBilateral, `iter_max`
    mean-field steps).  That library is not in this image; its published algorithm (Kraehenbuehl & Koltun 2011) is two
    permutohedral-lattice filters per step -- exactly what the bilateral regulariser of the training loop already runs on the device --
    around a softmax:   Q <- softmax(-U + pos_w K_g(Q) + bi_w K_b(Q)),   K(v) = n F(n v),  n = 1 / sqrt(F(1) + 1e-20)  (symmetric
    normalisation), F_g on the 2-D lattice of (x, y) / pos_xy_std, F_b on the 5-D lattice of (x, y) / bi_xy_std, rgb / bi_rgb_std.
    Checked in the test-suite against a CPU restatement of the same algorithm (parity with pydensecrf itself is unpinned: no fixture
    of its output exists).
    numpy in -> numpy out (the reference's types); CUDA tensors in -> CUDA tensor out."""

    def __init__(self, iter_max, pos_w, pos_xy_std, bi_w, bi_xy_std, bi_rgb_std):
        self.iter_max = iter_max
        self.pos_w = pos_w
        self.pos_xy_std = pos_xy_std
        self.bi_w = bi_w
        self.bi_xy_std = bi_xy_std
        self.bi_rgb_std = bi_rgb_std

    @staticmethod
    def _filter_gauss(v, sxy):
        K, H, W = v.shape
        L = _C.lib()
        ws = _C.workspace(L.cosa_lattice_filter_d2_workspace_bytes(1, K, H, W), v.device, "crf_d2")
        out = torch.empty_like(v)
        _C.check(L.cosa_lattice_filter_d2(_C.ptr(v), _C.ptr(out), 1, K, H, W, float(sxy), _C.ptr(ws), ws.numel(), _C.stream_ptr()),
                 "cosa_lattice_filter_d2")
        return out

    @staticmethod
    def _filter_bilateral(img, v, srgb, sxy):
        K, H, W = v.shape
        L = _C.lib()
        ws = _C.workspace(L.cosa_bilateral_workspace_bytes(1, K, H, W), v.device, "bilateral")
        out = torch.empty_like(v)
        _C.check(L.cosa_bilateralfilter_batch_dev(_C.ptr(img), _C.ptr(v), _C.ptr(out), 1, K, H, W, float(srgb), float(sxy), None, _C.ptr(ws),
                                                  ws.numel(), _C.stream_ptr()), "cosa_bilateralfilter_batch_dev")
        return out

    def __call__(self, image, probmap):
        as_numpy = not torch.is_tensor(probmap)
        dev = probmap.device if torch.is_tensor(probmap) and probmap.is_cuda else torch.device("cuda", torch.cuda.current_device())
        prob = torch.as_tensor(np.ascontiguousarray(probmap) if as_numpy else probmap).to(dev).float().contiguous()
        img = torch.as_tensor(np.ascontiguousarray(image) if not torch.is_tensor(image) else image).to(dev)
        C, H, W = prob.shape
        if img.shape != (H, W, 3):
            raise ValueError("DenseCRF: image must be [H, W, 3] (the reference passes the de-normalised uint8 image, HWC)")
        img = img.permute(2, 0, 1).float().contiguous()                                   # CHW planes 0..255, as the lattice kernels read them
        U = -torch.log(prob.clamp(1e-5, 1.0))                                             # pydensecrf.utils.unary_from_softmax
        one = torch.ones((1, H, W), device=dev)
        n_g = torch.rsqrt(self._filter_gauss(one, self.pos_xy_std) + 1e-20)
        n_b = torch.rsqrt(self._filter_bilateral(img, one, self.bi_rgb_std, self.bi_xy_std) + 1e-20)
        Q = torch.softmax(-U, dim=0)
        for _ in range(int(self.iter_max)):
            t = -U + float(self.pos_w) * (n_g * self._filter_gauss((Q * n_g).contiguous(), self.pos_xy_std)) \
                + float(self.bi_w) * (n_b * self._filter_bilateral(img, (Q * n_b).contiguous(), self.bi_rgb_std, self.bi_xy_std))
            Q = torch.softmax(t, dim=0)
        return Q.cpu().numpy() if as_numpy else Q


crf_inference_infv2 = DenseCRF(       # utils/seg_helper.py:989-996
    iter_max=1,
    pos_xy_std=1,
    pos_w=1,
    bi_xy_std=121,
    bi_rgb_std=5,
    bi_w=4,
)
