"""Latent-space maps under the reference's names: 2D / 3D scatter plots of ``model.encode`` latents reduced by incremental PCA or
t-SNE, for one model or for the (fused, video, 0D) latents of a multimodal one, and the 2D map over a decision-probability surface.

Signatures, defaults, the ``method`` spelling ('PCA' / 'tSNE'), the perplexities (64 in the single-model forms, 30 in the ``*_multi``
forms), colours, labels and figure layout are the reference's.  The latents are collected and reduced on the GPU
(src/visualization/_embed.py, csrc/embed.hip); only the finished (N, 2 | 3) embedding and the labels come to the host, where
matplotlib (imported inside the functions) draws them.  ``save_dir=None`` skips drawing.  Unlike the reference every function
returns what it drew: the embedding (or the (fused, video, 0D) triple of embeddings) as NumPy arrays and the integer labels.

Deviations: PCA equals ``IncrementalPCA.fit_transform`` to rounding, batching included.  t-SNE minimises the same objective with the
exact gradient and a deterministic PCA start instead of Barnes-Hut from a random one, so positions are not comparable with a
reference run (which does not reproduce itself either); the objective value and neighbourhood preservation are.
"""
from __future__ import annotations

from typing import Literal, Optional

import numpy as np
import torch
import torch.nn as nn

from . import _embed

COLORS = ("#1f77b4", "#ff7f0e")
NAMES = ("disruption", "normal")
SINGLE_PERPLEXITY = 64.0
MULTI_PERPLEXITY = 30.0
MULTI_TITLES = ("Embedded space for video + 0D data", "Embedded space for video data", "Embedded space for 0D data")


def _reduce(latent: torch.Tensor, nc: int, method: str, perplexity: float) -> np.ndarray:
    print("Dimension reduction process : start | latent vector : ({}, {})".format(latent.shape[0], latent.shape[1]))
    if method == "PCA":
        emb = _embed.pca_embed(latent, nc)
    else:
        emb, _ = _embed.tsne_embed(latent, nc, perplexity=perplexity)
    print("Dimension reduction process : complete")
    return emb.cpu().numpy()


def _scatter(ax, emb: np.ndarray, label: np.ndarray, order) -> None:
    for cls in order:
        pts = emb[label == cls]
        ax.scatter(*[pts[:, c] for c in range(emb.shape[1])], c=COLORS[cls], label=NAMES[cls])
    ax.set_xlabel("z-0")
    ax.set_ylabel("z-1")
    if emb.shape[1] == 3:
        ax.set_zlabel("z-2")
    ax.legend()


def _single(model, dataloader, device, save_dir, limit_iters, method, nc):
    latent, label = _embed.collect_latents(model, dataloader, device, limit_iters)
    emb = _reduce(latent, nc, method, SINGLE_PERPLEXITY)
    label = label.cpu().numpy().astype(int)
    if save_dir is not None:
        import matplotlib.pyplot as plt
        fig = plt.figure(figsize=(8, 6))
        ax = fig.add_subplot(projection="3d") if nc == 3 else fig.add_subplot()
        _scatter(ax, emb, label, (1, 0))
        fig.tight_layout()
        fig.savefig(save_dir)
        plt.close(fig)
    return emb, label


def _multi(model, dataloader, device, save_dir, limit_iters, method, nc):
    latents, label = _embed.collect_latents(model, dataloader, device, limit_iters, multi=True)
    embs = tuple(_reduce(v, nc, method, MULTI_PERPLEXITY) for v in latents)
    label = label.cpu().numpy().astype(int)
    if save_dir is not None:
        import matplotlib.pyplot as plt
        fig = plt.figure(figsize=(18, 8))
        for pos, (emb, title) in enumerate(zip(embs, MULTI_TITLES), start=1):
            ax = fig.add_subplot(1, 3, pos, projection="3d") if nc == 3 else fig.add_subplot(1, 3, pos)
            _scatter(ax, emb, label, (0, 1))
            ax.set_title(title)
        fig.tight_layout()
        fig.savefig(save_dir)
        plt.close(fig)
    return embs, label


def visualize_2D_latent_space(model: nn.Module, dataloader, device: str = "cpu", save_dir: Optional[str] = "./results/latent_2d_space.png",
                              limit_iters: int = 2, method: Literal["PCA", "tSNE"] = "PCA"):
    return _single(model, dataloader, device, save_dir, limit_iters, method, 2)


def visualize_3D_latent_space(model: nn.Module, dataloader, device: str = "cpu", save_dir: Optional[str] = "./results/latent_2d_space.png",
                              limit_iters: int = 2, method: Literal["PCA", "tSNE"] = "PCA"):
    return _single(model, dataloader, device, save_dir, limit_iters, method, 3)


def visualize_2D_latent_space_multi(model: nn.Module, dataloader, device: str = "cpu",
                                    save_dir: Optional[str] = "./results/fusion_latent_3d_space.png", limit_iters: int = 2,
                                    method: Literal["PCA", "tSNE"] = "PCA"):
    return _multi(model, dataloader, device, save_dir, limit_iters, method, 2)


def visualize_3D_latent_space_multi(model: nn.Module, dataloader, device: str = "cpu",
                                    save_dir: Optional[str] = "./results/fusion_latent_3d_space.png", limit_iters: int = 2,
                                    method: Literal["PCA", "tSNE"] = "PCA"):
    return _multi(model, dataloader, device, save_dir, limit_iters, method, 3)


def visualize_2D_decision_boundary(model: nn.Module, dataloader, device: str = "cpu",
                                   save_dir: Optional[str] = "./results/decision_boundary_2D_space.png", limit_iters: int = 2,
                                   method: Literal["PCA", "tSNE"] = "PCA"):
    """The 2D map drawn over the model's disruption probability, interpolated between the embedded points by a smoothing bivariate
    spline (scipy, on the host).  Returns (embedding, labels, probabilities of class 0)."""
    latent, label, probs = _embed.collect_latents(model, dataloader, device, limit_iters, with_probs=True)   # one pass over the loader
    probs = probs.cpu().numpy()
    emb = _reduce(latent, 2, method, SINGLE_PERPLEXITY)
    label = label.cpu().numpy().astype(int)
    if save_dir is not None:
        import matplotlib.pyplot as plt
        from scipy.interpolate import SmoothBivariateSpline
        gx, gy = np.meshgrid(emb[:, 0], emb[:, 1])
        surface = np.clip(SmoothBivariateSpline(emb[:, 0], emb[:, 1], probs)(gx, gy, grid=False), 0, 1)
        fig = plt.figure(figsize=(8, 6))
        ax = fig.add_subplot()
        ax.contourf(gx, gy, surface, levels=np.linspace(0, 1.0, 8), cmap=plt.cm.coolwarm)
        mp = plt.cm.ScalarMappable(cmap=plt.cm.coolwarm)
        mp.set_array(surface)
        mp.set_clim(0, 1.0)
        fig.colorbar(mp, ax=ax, boundaries=np.linspace(0, 1, 5))
        _scatter(ax, emb, label, (1, 0))
        fig.tight_layout()
        fig.savefig(save_dir)
        plt.close(fig)
    return emb, label, probs
