"""Input-gradient saliency on the MI355X: vanilla gradient and SmoothGrad maps of a class score with respect to the clip.

In the reference this is ``x.requires_grad_(); model.eval(); model(x)[:, target].backward(); x.grad`` (the first half of its
Grad-CAM tools, src/visualization/visualize_cam.py:81-85, taken down to the input).  Here the eval-mode backward is a chain of gfx950
kernels: for ``R2Plus1DClassifier`` the trunk executor's md_plan_input_grad is called directly on the forward that the plan's
eval workspace holds (no autograd graph); any other model whose units support the eval-mode backward (``SlowFast``) goes
through autograd.  The map kernel (md_saliency_map) reduces the channels and normalises per clip.

SmoothGrad (Smilkov et al. 2017): ``smooth = n`` noisy copies per clip, noise N(0, (sigma * (max - min of the clip))^2) drawn from
``generator`` in one call of shape (B, n, 3, T, H, W); the copies run through the model as batches of the clip batch's own size
(one plan serves all of them) and their gradients are averaged in copy order before the map.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from .. import ops
from . import _xai


class InputGradient:
    def __init__(self, model: nn.Module):
        self.model = model
        self.model.eval()

    # ------------------------------------------------------------------------------------------------------------------
    def _target_dlogits(self, logits: torch.Tensor, target) -> torch.Tensor:
        B, K = logits.shape
        if isinstance(target, torch.Tensor):
            tgt = target.to(device=logits.device, dtype=torch.int64).reshape(-1)
            if tgt.numel() != B:
                raise ValueError("target: %d entries for %d clips" % (tgt.numel(), B))
        else:
            if not 0 <= int(target) < K:
                raise ValueError("target %d outside [0, %d)" % (int(target), K))
            tgt = torch.full((B,), int(target), dtype=torch.int64, device=logits.device)
        return torch.zeros_like(logits).scatter_(1, tgt.view(-1, 1), 1.0)

    def gradient(self, video: torch.Tensor, target=0):
        """(d logit[b, target[b]] / d video (B,3,T,H,W), logits (B,K)) of the eval-mode model."""
        model = self.model
        if model.training:
            raise RuntimeError("InputGradient: the model is in training mode; saliency runs on the eval-mode forward")
        ops.require_cuda(video.contiguous())
        video = ops.f32(video.detach().contiguous())
        if hasattr(model, "res2plus1d") and hasattr(model, "linear"):
            trunk, head = model.res2plus1d, model.linear
            B, _, T, H, W = video.shape
            with torch.no_grad():
                feat = trunk(video)                   # no autograd node: the plan's eval workspace holds the activations
                logits = head(feat)
                lin0, bn, act, lin1 = head[0], head[1], head[2], head[3]
                alpha = float(act.alpha) if isinstance(act, nn.ELU) else -float(act.negative_slope)
                dfeat = _xai.head_eval_bwd(feat, lin0, bn, lin1, alpha, self._target_dlogits(logits, target))
                plan = trunk._plan(B, T, H, W)
                dx, _ = plan.input_grad(dfeat, plan.eval_workspace(video.device), [u.conv.weight for u in trunk.unit_modules()])
            return dx, logits
        x = video.clone().requires_grad_(True)
        with torch.enable_grad():
            logits = model(x)
            (logits * self._target_dlogits(logits.detach(), target)).sum().backward()
        return x.grad.detach(), logits.detach()

    @staticmethod
    def noisy_copies(video: torch.Tensor, n: int, sigma: float, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """(n, B, 3, T, H, W): copy j of clip b is video[b] + sigma * (max - min of clip b) * noise[b, j]."""
        B = video.shape[0]
        noise = torch.randn((B, n) + tuple(video.shape[1:]), device=video.device, dtype=torch.float32, generator=generator)
        flat = video.reshape(B, -1)
        span = (flat.max(1)[0] - flat.min(1)[0]).view(B, 1, 1, 1, 1, 1)
        return (video.unsqueeze(1) + float(sigma) * span * noise).transpose(0, 1).contiguous()

    def compute(self, video: torch.Tensor, target=0, mode: str = "max", smooth: int = 0, sigma: float = 0.0,
                generator: Optional[torch.Generator] = None):
        """video (B,3,T,H,W) on the GPU -> (grad (B,3,T,H,W), maps (B,T,H,W) in [0,1], logits (B,K) of the clean clips)."""
        if mode not in _xai.SALIENCY_MODE:
            raise ValueError("mode must be one of %s, got %r" % (sorted(_xai.SALIENCY_MODE), mode))
        smooth = int(smooth)
        if smooth < 0:
            raise ValueError("smooth must be >= 0")
        video = ops.f32(video.detach().contiguous())
        if smooth == 0:
            grad, logits = self.gradient(video, target)
        else:
            copies = self.noisy_copies(video, smooth, sigma, generator)
            with torch.no_grad():
                logits = self.model(video)
            grad = None
            for j in range(smooth):                          # batches of the clip batch's own shape: one plan, fixed order
                g, _ = self.gradient(copies[j], target)
                grad = g if grad is None else grad.add_(g)
            grad = grad / float(smooth)
        return grad, _xai.saliency_map(grad, mode), logits
