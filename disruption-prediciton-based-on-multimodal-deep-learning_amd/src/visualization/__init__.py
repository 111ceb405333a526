"""Explainability tools of the reference's ``src/visualization`` on the MI355X: ``visualize_cam.GradCAM_R2Plus1D`` /
``GradCAM_SlowFast``, ``visualize_attention.ViViTAttentionRollout`` and ``visualize_saliency.InputGradient`` (maps computed by the
gfx950 kernels of csrc/xai.hip and csrc/eval_bwd.hip, batched over clips), and the latent-space maps of
``visualize_latent_space`` (incremental PCA and exact t-SNE on the GPU, csrc/embed.hip)."""
import os as _os

_ref = _os.environ.get("MD_REFERENCE_SRC")
if _ref and _os.path.isdir(_os.path.join(_ref, "visualization")):
    __path__.append(_os.path.join(_ref, "visualization"))
