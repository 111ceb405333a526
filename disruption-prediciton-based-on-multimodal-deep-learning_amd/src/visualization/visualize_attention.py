"""Attention rollout for ViViT (reference src/visualization/visualize_attention.py:28-135) on the MI355X, batched over clips.

The reference hooks every ``{space,temporal}_transformer.layers.{i}.0.fn.to_qkv``; here qkv is computed without calling that module,
so the matched ``Attention`` modules are armed with a recorder for the duration of one forward instead.  While armed, each of them
hands the qkv it already has to md_attention_probs_fused, which writes the head-fused (B, S, S) probabilities (the per-head matrices
never reach memory).  Unarmed, ``Attention.forward`` is unchanged.  The rollout is then three kernels: md_rollout_discard,
md_rollout_chain and md_rollout_mask.

Quirk kept: the reference zeroes the discarded entries of the FIRST sequence of the batch only (``flat[0, indices] = 0``, the union
of every sequence's k smallest entries, index 0 excepted); the paper's figures were made that way, so here it is the first sequence
of every clip.  Ties at the k-th smallest value are taken in ascending flat index order (exactly k per sequence, as torch.topk).
Deviation: an unknown ``head_fusion`` raises ValueError (the reference raises a string, a TypeError).
"""
from __future__ import annotations

from typing import List, Literal

import numpy as np
import torch
import torch.nn as nn

from ..models.ViViT import Attention
from . import _xai


def rollout_from_fused(fused_layers: torch.Tensor, n_clips: int, discard_ratio: float, kind: int):
    """fused_layers (L, n_seq, S, S): the head-fused maps of one transformer, n_seq = n_clips * sequences per clip (frames for the
    space transformer, 1 for the temporal one) -> (discarded maps, rollout (n_seq, S, S), mask of md_rollout_mask)."""
    L, nseq, S, _ = fused_layers.shape
    if nseq % n_clips:
        raise ValueError("%d sequences do not split into %d clips" % (nseq, n_clips))
    k = int(S * S * discard_ratio)                     # the reference's own rounding: int(flat.size(-1) * discard_ratio)
    disc = _xai.rollout_discard(fused_layers, nseq // n_clips, k)
    result = _xai.rollout_chain(disc)
    return disc, result, _xai.rollout_mask(result, n_clips, kind)


class ViViTAttentionRollout:
    def __init__(self, model: nn.Module, layer_name='0.fn.to_qkv', head_fusion='mean', discard_ratio=0.9,
                 transformer: Literal['temporal', 'space'] = 'space'):
        if head_fusion not in _xai.FUSION:
            raise ValueError("Attention head fusion type %r not supported (mean, max or min)" % (head_fusion,))
        self.model = model
        self.head_fusion = head_fusion
        self.discard_ratio = discard_ratio
        self.module_name = "space_transformer" if transformer == 'space' else "temporal_transformer"
        modules = dict(model.named_modules())
        self._armed: List[Attention] = []
        for name, module in model.named_modules():
            if layer_name in name and self.module_name in name:
                parent = modules.get(name.rsplit(".", 1)[0]) if "." in name else None
                if not (name.endswith(".to_qkv") and isinstance(parent, Attention)):
                    raise ValueError("%s: only the to_qkv projections of ViViT Attention modules can be recorded" % name)
                self._armed.append(parent)
        if not self._armed:
            raise ValueError("no module of %s matches %r" % (self.module_name, layer_name))
        self.attentions: List[torch.Tensor] = []
        self._buf = None

    def _record(self, module: Attention, qkv: torch.Tensor):
        B, S, _ = qkv.shape
        i = len(self.attentions)
        if self._buf is None:
            self._buf = torch.empty((len(self._armed), B, S, S), device=qkv.device)
        if i >= self._buf.shape[0] or self._buf.shape[1:] != (B, S, S):
            raise RuntimeError("ViViTAttentionRollout: unexpected attention call %d with (B, S) = (%d, %d)" % (i, B, S))
        self.attentions.append(_xai.attention_probs_fused(qkv, module.n_heads, self.head_fusion, True, out=self._buf[i]))

    def __call__(self, input_tensor: torch.Tensor):
        """The reference's NumPy mask for one clip -- (T, w, w) for the space transformer, (T, T) for the temporal one -- with a
        leading clip axis for a batch."""
        self.attentions, self._buf = [], None
        for m in self._armed:
            m._xai_recorder = self._record
        try:
            with torch.no_grad():
                self.model(input_tensor)
        finally:
            for m in self._armed:
                m._xai_recorder = None
        if len(self.attentions) != len(self._armed):
            raise RuntimeError("ViViTAttentionRollout: %d of %d armed layers ran" % (len(self.attentions), len(self._armed)))
        B = input_tensor.shape[0]
        space = self.module_name == "space_transformer"
        _, _, mask = rollout_from_fused(self._buf, B, self.discard_ratio, 0 if space else 1)
        if space:
            width = int((mask.shape[-1]) ** 0.5)
            mask = mask.reshape(B, mask.shape[1], width, width)
        else:
            mask = mask.reshape(B, mask.shape[-2], mask.shape[-1])
        mask = mask.cpu().numpy()
        return mask[0] if B == 1 else mask


def visualize_spatio_attention(shot: np.ndarray, att_map: np.ndarray, size: int = 128, save_dir="./results/spatio_attention.png"):
    """Plot a frame beside its (n_h, n_w) space mask resized to size x size (bilinear, as the reference's cv2.resize)."""
    import matplotlib.pyplot as plt
    t = torch.as_tensor(np.asarray(att_map, dtype=np.float32))[None, None]
    att = torch.nn.functional.interpolate(t, size=(size, size), mode="bilinear", align_corners=False)[0, 0].numpy()
    fig, (ax1, ax2) = plt.subplots(ncols=2, figsize=(16, 16))
    ax1.set_title('Original')
    ax2.set_title('Attention Map Last Layer')
    ax1.imshow(shot)
    ax2.imshow(att)
    fig.savefig(save_dir)
    return fig


def visualize_temporal_attention(att_map: np.ndarray, save_dir: str = "./result/temporal_attention.png"):
    """Plot a (T, T) temporal mask with a colour bar."""
    import matplotlib.pyplot as plt
    fig = plt.figure(figsize=(6, 3.2))
    ax = fig.add_subplot(111)
    ax.set_title('Temporal attention mask')
    im = ax.imshow(att_map)
    ax.set_aspect('equal')
    fig.colorbar(im, ax=ax, orientation='vertical')
    fig.savefig(save_dir)
    return fig
