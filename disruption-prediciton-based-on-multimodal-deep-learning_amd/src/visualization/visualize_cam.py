"""Grad-CAM for R(2+1)D (reference src/visualization/visualize_cam.py:57-132) on the MI355X, batched over clips.

The reference hooks ``res2plus1d.conv5``; here the trunk runs as one executor plan and conv5 is never called as a module, so the
map is computed from what the plan already holds.  conv5's output is the last tensor the executor materialises (the one the average
pool reads) and the pool is the only op after it, so the gradient of the score there is dfeat / (T'*h*w) at every position: no trunk
backward is needed, only the eval-mode input gradient of the head (md_head_eval_dfeat) and one map kernel pair (md_gradcam).

Deviations from the reference: a clip whose map is constant (all zero after the ReLU, say) gets an all-zero map where the reference
divides 0 by 0; the map has the clip's own size and frame count instead of the hard-coded 3 x 8 x 8 -> 128 x 128; its misspelt
gradient list and the axes used before ``plt.subplots`` are not reproduced.

``GradCAM_SlowFast`` (reference visualize_cam.py:136-282) takes its two maps at the raw output of
``encoder.slownet.layer4[0].downsample[0]`` (the Conv3d, before its BatchNorm) and at the output of ``encoder.fastnet.l_layer3``.
No module hooks: the eval-mode backward of those two units hands out the activation and its gradient (``_unit.capture_units``),
and the maps use the tensors' own shapes instead of the reference's ``view(1,1,5,4,4)`` / ``(1,1,5,8,8)`` and 512 / 64 channels.

``layer="conv1" ... "conv4"`` (an addition: the reference hooks conv5 only) takes the map at an earlier, finer layer.  There the
gradient is not uniform, so the eval-mode backward of the plan runs down to that layer's output (md_plan_input_grad with stop_z)
and md_gradcam_grad forms the channel weights as the mean of that gradient, as visualize_cam.py:87-90 does.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from .. import _native as N
from .. import ops
from . import _xai


def _jet_bgr() -> np.ndarray:
    """256 x 3 uint8 JET table in OpenCV's BGR channel order, standing in for cv2.applyColorMap(..., cv2.COLORMAP_JET): the
    piecewise-linear jet ramp (blue -> cyan -> yellow -> red).  PARITY UNPINNED: OpenCV is not a dependency and its own table is
    interpolated from control points, so single entries may differ from it by a few levels."""
    x = np.arange(256, dtype=np.float64) / 255.0
    r = np.clip(1.5 - np.abs(4.0 * x - 3.0), 0.0, 1.0)
    g = np.clip(1.5 - np.abs(4.0 * x - 2.0), 0.0, 1.0)
    b = np.clip(1.5 - np.abs(4.0 * x - 1.0), 0.0, 1.0)
    return np.round(255.0 * np.stack([b, g, r], axis=-1)).astype(np.uint8)


JET_BGR = _jet_bgr()


def apply_color_map_jet(img_u8: np.ndarray) -> np.ndarray:
    """(H, W) uint8 -> (H, W, 3) uint8 BGR through JET_BGR."""
    return JET_BGR[np.asarray(img_u8, dtype=np.uint8)]


class GradCAM_R2Plus1D:
    LAYERS = ("conv1", "conv2", "conv3", "conv4", "conv5")

    def __init__(self, model: nn.Module, layer: str = "conv5"):
        super().__init__()
        self.model = model
        for name in ("res2plus1d", "linear"):
            if not hasattr(model, name):
                raise ValueError("GradCAM_R2Plus1D needs an R2Plus1DClassifier (no `%s` child)" % name)
        if layer not in self.LAYERS:
            raise ValueError("layer must be one of %s, got %r" % (self.LAYERS, layer))
        self.layer = layer
        self.general = False      # True: layer "conv5" also goes through the general path (plan backward + md_gradcam_grad)
        self.model.eval()

    def _layer_z(self, plan):
        """(index of the materialised tensor that is this layer's output, (T', h, w) there)."""
        ls = self.model.res2plus1d.layer_sizes
        k = self.LAYERS.index(self.layer)
        if k == 0:
            d = plan.descs[1]
            return 1, (d.To, d.Ho, d.Wo)
        ui, z = 2, 1
        for st in range(4):
            for bi in range(ls[st]):
                down = bi == 0 and st > 0
                last = ui + 3                      # conv2.temporal_conv of this block
                ui += 6 if down else 4
                z += 1
            if st + 1 == k:
                d = plan.descs[last]
                return z, (d.To, d.Ho, d.Wo)
        raise AssertionError

    def compute(self, video: torch.Tensor, target=0):
        """video (B, 3, T, H, W) on the GPU -> (maps (B, H, W) in [0, 1], logits (B, K)), target an int or a (B,) tensor of
        classes.  ``self.cam_raw`` keeps the last ReLU'd map before the resize, (B, T', h, w)."""
        model = self.model
        if model.training:
            raise RuntimeError("GradCAM_R2Plus1D: the model is in training mode; Grad-CAM runs on the eval-mode forward")
        trunk, head = model.res2plus1d, model.linear
        ops.require_cuda(video.contiguous())
        video = ops.f32(video.contiguous())
        B, _, T, H, W = video.shape
        with torch.no_grad():
            feat = trunk(video)                       # no autograd node: the plan's eval workspace holds the activations
            logits = head(feat)
            lin0, bn, act, lin1 = head[0], head[1], head[2], head[3]
            alpha = float(act.alpha) if isinstance(act, nn.ELU) else -float(act.negative_slope)
            dfeat = _xai.head_eval_dfeat(feat, lin0, bn, lin1, alpha, target)
            plan = trunk._plan(B, T, H, W)
            ws = plan.eval_workspace(video.device)
            if self.layer != "conv5" or self.general:
                # the gradient at this layer from the eval-mode backward of the plan; same stream, so the eval workspace still
                # holds this forward
                zi, (Tq, hq, wq) = self._layer_z(plan)
                _, dz = plan.input_grad(dfeat, ws, [u.conv.weight for u in trunk.unit_modules()], want_dx=False, stop_z=zi)
                z, C = plan.z_tensor(ws, zi)
                self.dz, self.act = dz, z
                self.weights, self.cam_raw, maps = _xai.gradcam_grad(z, dz, C, B, Tq, hq, wq, H, W)
                return maps, logits
            # conv5's output read in place, where the executor left it.  This must be queued before any later forward at this
            # shape reuses the eval workspace (same stream, so ordering on the device is then guaranteed).
            z, C = plan.z_tensor(ws, N.lib().md_plan_num_z(plan._h) - 1)
            last = plan.descs[-1]
            self.cam_raw, maps = _xai.gradcam(z, C, last.To, last.Ho, last.Wo, dfeat, H, W)
        return maps, logits

    def __call__(self, video: torch.Tensor, title: Optional[str] = None, save_dir: Optional[str] = None):
        """The reference's (img, grad_heatmap, grad_result, fig) for one clip; fig is None when matplotlib is not installed."""
        if video.shape[0] != 1:
            raise ValueError("GradCAM_R2Plus1D.__call__ takes one clip (as the reference); use compute() for a batch")
        maps, _ = self.compute(video, 0)
        grad_cam_map = maps[0].cpu().numpy()
        grad_heatmap = apply_color_map_jet(np.uint8(255 * grad_cam_map))
        img = video[:, :, -1, :, :].squeeze().permute(1, 2, 0).detach().cpu().numpy()
        grad_result = grad_heatmap + img
        grad_result = grad_result / np.max(grad_result)
        grad_result = np.uint8(255 * grad_result)
        fig = None
        try:
            import matplotlib.pyplot as plt
        except ImportError:
            plt = None
        if plt is not None:
            fig, (ax1, ax2, ax3) = plt.subplots(ncols=3, figsize=(12, 8))
            ax1.set_title('Original - {}'.format(title) if title else 'Original')
            ax2.set_title('GradCAM - {}'.format(title) if title else 'GradCAM')
            ax1.imshow(img)
            ax2.imshow(grad_heatmap)
            ax3.imshow(grad_result)
            fig.tight_layout()
            if save_dir:
                fig.savefig(save_dir)
        return img, grad_heatmap, grad_result, fig


class GradCAM_SlowFast:
    def __init__(self, model: nn.Module):
        super().__init__()
        self.model = model
        try:
            self.slow_conv = model.encoder.slownet.layer4[0].downsample[0]
            self.fast_conv = model.encoder.fastnet.l_layer3
        except (AttributeError, TypeError, IndexError):
            raise ValueError("GradCAM_SlowFast needs a SlowFast model (encoder.slownet.layer4[0].downsample[0], encoder.fastnet.l_layer3)")
        self.model.eval()

    def compute(self, video: torch.Tensor, target=0):
        """video (B, 3, T, H, W) on the GPU -> (maps_slow (B, H, W), maps_fast (B, H, W), logits (B, K)).  Kept from the last
        call: ``act`` / ``grad`` / ``weights`` / ``cam_raw``, dicts over "slow" and "fast" (activation and gradient channels-last
        [B, T', h, w, cpad(C)]), and ``input_grad`` (B, 3, T, H, W), which the backward produces on the way."""
        from ..models import _unit
        model = self.model
        if model.training:
            raise RuntimeError("GradCAM_SlowFast: the model is in training mode; Grad-CAM runs on the eval-mode forward")
        ops.require_cuda(video.contiguous())
        x = ops.f32(video.detach().contiguous()).clone().requires_grad_(True)      # the chain reaches a unit only through its input
        B, _, T, H, W = x.shape
        with _unit.capture_units({"slow": self.slow_conv.weight, "fast": self.fast_conv.weight}) as cap, torch.enable_grad():
            logits = model(x)
            K = logits.shape[1]
            if isinstance(target, torch.Tensor):
                tgt = target.to(device=x.device, dtype=torch.int64).reshape(-1)
                if tgt.numel() != B:
                    raise ValueError("target: %d entries for %d clips" % (tgt.numel(), B))
            else:
                if not 0 <= int(target) < K:
                    raise ValueError("target %d outside [0, %d)" % (int(target), K))
                tgt = torch.full((B,), int(target), dtype=torch.int64, device=x.device)
            logits.gather(1, tgt.view(-1, 1)).sum().backward()
        torch.cuda.synchronize(x.device)           # the fast pathway may have run on a side stream
        self.input_grad = x.grad.detach()
        self.act, self.grad, self.weights, self.cam_raw, maps = {}, {}, {}, {}, {}
        for name in ("slow", "fast"):
            if name not in cap.out:
                raise RuntimeError("GradCAM_SlowFast: the backward did not pass through the %s pathway's hooked convolution" % name)
            act, grad, C = cap.out[name]
            act, grad = act.detach(), grad.detach()
            _, Tq, h, w, Cp = act.shape
            self.act[name], self.grad[name] = act, grad
            self.weights[name], self.cam_raw[name], maps[name] = _xai.gradcam_grad(act.reshape(-1, Cp), grad.reshape(-1, Cp), C, B, Tq, h,
                                                                                   w, H, W)
        return maps["slow"], maps["fast"], logits.detach()

    def __call__(self, video: torch.Tensor, title: Optional[str] = None, save_dir: Optional[str] = None):
        """The reference's (img, grad_heatmap_sn, grad_heatmap_fn, fig) for one clip; fig is None when matplotlib is not installed."""
        if video.shape[0] != 1:
            raise ValueError("GradCAM_SlowFast.__call__ takes one clip (as the reference); use compute() for a batch")
        ms, mf, _ = self.compute(video, 0)
        grad_heatmap_sn = apply_color_map_jet(np.uint8(255 * ms[0].cpu().numpy()))
        grad_heatmap_fn = apply_color_map_jet(np.uint8(255 * mf[0].cpu().numpy()))
        img = video[:, :, -1, :, :].squeeze().permute(1, 2, 0).detach().cpu().numpy()
        fig = None
        try:
            import matplotlib.pyplot as plt
        except ImportError:
            plt = None
        if plt is not None:
            fig, (ax1, ax2, ax3) = plt.subplots(ncols=3, figsize=(12, 8))
            ax1.set_title('Original - {}'.format(title) if title else 'Original')
            ax2.set_title('GradCAM(Slow) - {}'.format(title) if title else 'GradCAM(Slow)')
            ax3.set_title('GradCAM(Fast) - {}'.format(title) if title else 'GradCAM(Fast)')
            ax1.imshow(img)
            ax2.imshow(grad_heatmap_sn)
            ax3.imshow(grad_heatmap_fn)
            fig.tight_layout()
            if save_dir:
                fig.savefig(save_dir)
        return img, grad_heatmap_sn, grad_heatmap_fn, fig
