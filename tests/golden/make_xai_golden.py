#!/usr/bin/env python3
"""Generate the explainability fixtures (xai_*.npz) in this directory from the REFERENCE implementation.

Run in the build container only (needs the reference checkout; never on the GPU box):

    python tests/golden/make_xai_golden.py

As in make_golden.py the reference is imported unmodified, with empty stand-ins in ``sys.modules`` for modules that play no part
in the arithmetic; ``cv2`` is one of them (the tools only use it for colouring and resizing pictures).

Grad-CAM: a reference R2Plus1DClassifier([1,1,1,1]) in eval mode, parameters from ``oracle/r2plus1d.py::synth_state``, with a
forward hook and a full backward hook on ``res2plus1d.conv5``; the score is logit[:, 0].  Recorded: conv5's output and its
gradient, the channel weights alpha, the ReLU'd map and the normalised map.  The map step after the hooks is restated here (the
reference's own step hard-codes a 3 x 8 x 8 map and cannot run).  The clips are ``clip()`` below (synth_clip's recipe with a
rectangular frame), so a test regenerates them from the seed.

Rollout: reference ViViT models (seeded init as make_golden.py's vivit_fixture), eval mode, run through the reference's own
ViViTAttentionRollout for the space and the temporal transformer and each head fusion.  Recorded: the state dict, the clip, the
per-layer head-fused maps before the discard step (all sequences) and after it (the first sequence, the only one it changes), and
the masks the reference returns.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("REFERENCE_ROOT", "/root/reference")


def _stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


_stub("pytorch_model_summary", summary=lambda *a, **k: "")
_stub("seaborn")
_stub("cv2", COLORMAP_JET=2)

sys.path.insert(0, REF)     # the reference's own `src` package
sys.path.insert(1, ROOT)    # oracle/ (weight recipes only)

import matplotlib                                   # noqa: E402
matplotlib.use("Agg")

from oracle import r2plus1d as orc                  # noqa: E402
from src.models.R2Plus1D import R2Plus1DClassifier  # noqa: E402  (reference)
from src.models.ViViT import ViViT                  # noqa: E402  (reference)
from src.visualization import visualize_attention as ref_va   # noqa: E402  (reference)

torch.set_num_threads(8)

CAM_CASES = (("cam_a", 21, 128, 128, 1101), ("cam_b", 12, 96, 80, 1103))
ROLLOUT_CASES = (("roll17", 32, 5, 81), ("roll65", 64, 3, 85))


def clip(B, T, H, W, seed):
    """synth_clip's recipe for (B, 3, T, H, W): uniform integers in [0, 255] minus the BGR means."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, size=(B, 3, T, H, W)).astype("float32")
    x -= np.array([90.0, 98.0, 102.0], dtype="float32").reshape(1, 3, 1, 1, 1)
    return torch.from_numpy(x)


def cam_map(act, grad, H, W):
    """Grad-CAM map step (visualize_cam.py:87-103 without its fixed sizes): act, grad (1, C, T', h, w) -> alpha, raw, map."""
    C = act.shape[1]
    alpha = grad.mean(2).reshape(1, C, -1).mean(2)
    raw = torch.relu((alpha.reshape(1, C, 1, 1, 1) * act).sum(1))                                   # (1, T', h, w)
    frames = torch.nn.functional.interpolate(raw.permute(1, 0, 2, 3), size=(H, W), mode="bilinear", align_corners=False)
    m = frames.mean(0)[0]
    lo, hi = m.min(), m.max()
    return alpha, raw, (m - lo) / (hi - lo)


def cam_fixture(tag, T, H, W, seed, alpha=0.01):
    ls = [1, 1, 1, 1]
    model = R2Plus1DClassifier(input_size=(3, T, H, W), num_classes=2, layer_sizes=ls, alpha=alpha)
    params, bufs = orc.synth_state(ls, seed, alpha)
    sd = dict(params); sd.update(bufs)
    missing, unexpected = model.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    model.eval()
    acts, grads = [], []
    conv5 = model.res2plus1d.conv5
    conv5.register_forward_hook(lambda m, i, o: acts.append(o.detach()))
    conv5.register_full_backward_hook(lambda m, gi, go: grads.append(go[0].detach()))
    x = clip(1, T, H, W, seed).requires_grad_(True)
    logit = model(x)
    logit[:, 0].squeeze().backward()
    act, grad = acts[-1], grads[-1]
    a, raw, m = cam_map(act, grad, H, W)
    print(tag, tuple(act.shape), "map range", float(m.min()), float(m.max()))
    np.savez_compressed(os.path.join(HERE, "xai_%s.npz" % tag), seed=np.int64(seed), shape=np.array([T, H, W]),
                        slope=np.float32(alpha), logits=logit.detach().numpy(), act=act.numpy(), grad=grad.numpy(),
                        alpha=a.numpy(), cam_raw=raw.numpy(), map=m.numpy())


def _fuse(att, how):
    return att.mean(1) if how == "mean" else (att.max(1)[0] if how == "max" else att.min(1)[0])


def rollout_fixture(tag, image, n_frames, seed):
    torch.manual_seed(seed)
    m = ViViT(image_size=image, patch_size=8, n_frames=n_frames, n_classes=2, dim=32, depth=2, n_heads=2, pool="cls", in_channels=3,
              d_head=16, dropout=0.0, embedd_dropout=0.0, scale_dim=2, alpha=0.7)
    with torch.no_grad():
        for k, v in m.named_parameters():
            if "norm" in k or k.startswith("mlp.1"):
                (v.uniform_(0.5, 1.5) if k.endswith("weight") else v.normal_(0, 0.3))
    m.eval()
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(1, n_frames, 3, image, image, generator=g)
    rec = {"x": x.numpy(), "discard_ratio": np.float32(0.9)}
    for k, v in m.state_dict().items():
        rec["sd/" + k] = v.numpy()
    for tr in ("space", "temporal"):
        for how in ("mean", "max", "min"):
            ro = ref_va.ViViTAttentionRollout(m, head_fusion=how, discard_ratio=0.9, transformer=tr)
            mask = ro(x)
            fused = torch.stack([_fuse(a, how) for a in ro.attentions])                 # (L, n_seq, S, S)
            L, nseq, S, _ = fused.shape
            after = fused[:, 0].clone().reshape(L, -1)
            for l in range(L):                                                          # the discard step, restated
                _, idx = fused[l].reshape(nseq, -1).topk(int(S * S * 0.9), dim=-1, largest=False)
                idx = idx[idx != 0]
                after[l, idx] = 0
            key = "%s/%s/" % (tr, how)
            rec[key + "fused"] = fused.numpy()
            rec[key + "first_after"] = after.reshape(L, S, S).numpy()
            rec[key + "mask"] = np.asarray(mask, dtype=np.float32)
            for h in ro.model.modules():
                h._forward_hooks.clear()
            print(tag, tr, how, tuple(fused.shape), np.asarray(mask).shape)
    np.savez_compressed(os.path.join(HERE, "xai_%s.npz" % tag), **rec)


if __name__ == "__main__":
    for case in CAM_CASES:
        cam_fixture(*case)
    for case in ROLLOUT_CASES:
        rollout_fixture(*case)
    for f in sorted(os.listdir(HERE)):
        if f.startswith("xai_"):
            print(f, os.path.getsize(os.path.join(HERE, f)))
