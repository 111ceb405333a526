"""CPU tests of the eval-mode backward feature: the oracle's eval-mode input gradient against the reference recordings
(tests/golden/sal_*.npz, written by tests/golden/make_saliency_golden.py), float64 restatements of md_saliency_map and
md_gradcam_grad (what tests/test_saliency_gpu.py compares the kernels with) against the recorded maps, the header <-> binding <->
library check for the new symbols, and the constructor contract of the visualisation classes."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import r2plus1d as orc
from oracle import slowfast as osf
from src import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_num_threads(8)

NEW_SYMBOLS = ("md_bn_eval_bwd", "md_residual_eval_bwd", "md_stem_dgrad_supported", "md_stem_dgrad", "md_plan_input_grad",
               "md_head_eval_bwd", "md_gradcam_grad_scratch_floats", "md_gradcam_grad", "md_saliency_scratch_floats",
               "md_saliency_map")


def clip(B, T, H, W, seed):
    """make_saliency_golden.py::clip."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, size=(B, 3, T, H, W)).astype("float32")
    x -= np.array([90.0, 98.0, 102.0], dtype="float32").reshape(1, 3, 1, 1, 1)
    return torch.from_numpy(x)


def load(golden_dir, tag):
    return np.load(os.path.join(golden_dir, "sal_%s.npz" % tag))


def rel_max(a, b):
    """max|a - b| / max|b| (the absolute difference when b is all zero)."""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b))) / (float(np.max(np.abs(b))) or 1.0)


def recorded_map(m):
    """A recorded map; the reference's 0/0 for a constant map (all NaN) is the all-zero map here (the project's stated deviation)."""
    m = np.asarray(m, dtype=np.float64)
    return np.zeros_like(m) if np.isnan(m).all() else m


# ---------------------------------------------------------------------------------------------------------- restatements (fp64)
def saliency_map_ref(dx, mode="max"):
    """md_saliency_map: dx (B, C, T, H, W) -> (B, T, H, W); max | sum over channels of |dx|, per-clip min-max, constant -> zeros."""
    a = np.abs(np.asarray(dx, dtype=np.float64))
    m = a.max(1) if mode == "max" else a.sum(1)
    out = np.zeros_like(m)
    for b in range(m.shape[0]):
        lo, hi = m[b].min(), m[b].max()
        if hi > lo:
            out[b] = (m[b] - lo) / (hi - lo)
    return out


def bilinear_resize(frames, OH, OW):
    """F.interpolate(mode="bilinear", align_corners=False) of (N, h, w) frames, in float64."""
    frames = np.asarray(frames, dtype=np.float64)
    _, h, w = frames.shape
    sy = np.maximum((np.arange(OH) + 0.5) * (h / OH) - 0.5, 0.0); sx = np.maximum((np.arange(OW) + 0.5) * (w / OW) - 0.5, 0.0)
    y0 = np.floor(sy).astype(int); x0 = np.floor(sx).astype(int)
    y1 = np.minimum(y0 + 1, h - 1); x1 = np.minimum(x0 + 1, w - 1)
    ly = (sy - y0)[None, :, None]; lx = (sx - x0)[None, None, :]
    f = frames
    top = f[:, y0][:, :, x0] * (1 - lx) + f[:, y0][:, :, x1] * lx
    bot = f[:, y1][:, :, x0] * (1 - lx) + f[:, y1][:, :, x1] * lx
    return top * (1 - ly) + bot * ly


def gradcam_grad_ref(act, dact, OH, OW):
    """md_gradcam_grad: act, dact (B, C, T', h, w) -> (weights (B, C), cam_raw (B, T', h, w), map (B, OH, OW))."""
    act = np.asarray(act, dtype=np.float64); dact = np.asarray(dact, dtype=np.float64)
    wts = dact.mean(axis=(2, 3, 4))
    raw = np.maximum((wts[:, :, None, None, None] * act).sum(1), 0.0)
    maps = np.zeros((act.shape[0], OH, OW))
    for b in range(act.shape[0]):
        m = bilinear_resize(raw[b], OH, OW).mean(0)
        lo, hi = m.min(), m.max()
        if hi > lo:
            maps[b] = (m - lo) / (hi - lo)
    return wts, raw, maps


# ---------------------------------------------------------------------------------------------------------- oracle vs recordings
def oracle_r2p1d(g, B=None, force=None, tap=None):
    ls = [int(v) for v in g["layer_sizes"]]
    Bf, T, H, W = (int(v) for v in g["shape"])
    seed, slope = int(g["seed"]), float(g["slope"])
    params, bufs = orc.synth_state(ls, seed, slope)
    sd = {k: v.double() for k, v in params.items()}
    b64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in bufs.items()}
    x = clip(B or Bf, T, H, W, seed).double().requires_grad_(True)
    logits = orc.classifier_forward(x, sd, b64, ls, slope, training=False, tap=tap, force=force)
    dx, = torch.autograd.grad(logits[:, 0].sum(), x)
    return logits.detach(), dx


@pytest.mark.parametrize("tag", ["r2p1d_a", "r2p1d_lin"])
def test_oracle_eval_input_gradient_matches_reference_recording(golden_dir, tag):
    g = load(golden_dir, tag)
    logits, dx = oracle_r2p1d(g)
    print(tag, "logits", rel_max(logits.numpy(), g["logits"]), "dx", rel_max(dx.numpy(), g["dx"]), "reference fp32 vs fp64",
          float(g["self32/dx"]))
    assert rel_max(logits.numpy(), g["logits"]) <= 1e-5
    assert rel_max(dx.numpy(), g["dx"]) <= 1e-5
    assert float(g["self32/dx"]) < 1e-5          # the recording is free of sign flips between the reference's fp32 and fp64 runs


def slowfast_state(g, dtype=torch.float64):
    from src.models.slowfast import SlowFast                       # the mirror builds on the CPU; only its forward needs the GPU
    layers = [int(v) for v in g["layers"]]
    B, T, S, _ = (int(v) for v in g["shape"])
    m = SlowFast(input_shape=(3, T, S, S), layers=layers, alpha=4, tau_fast=1, num_classes=2, alpha_elu=1.0)
    sd = osf.synth_state({k: tuple(v.shape) for k, v in m.state_dict().items()}, int(g["seed"]))
    return m, sd, layers, osf.synth_clip(B, T, S, int(g["seed"]) + 1)


def test_slowfast_oracle_eval_input_gradient_matches_reference_recording(golden_dir):
    g = load(golden_dir, "slowfast")
    _, sd, layers, x = slowfast_state(g)
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    x = x.double().requires_grad_(True)
    logits = osf.slowfast_forward(x, sd64, layers, 4, 1, 1.0, False)
    dx, = torch.autograd.grad(logits[:, 0].sum(), x)
    print("slowfast logits", rel_max(logits.detach().numpy(), g["logits"]), "dx", rel_max(dx.numpy(), g["dx"]))
    assert rel_max(logits.detach().numpy(), g["logits"]) <= 1e-5
    assert rel_max(dx.numpy(), g["dx"]) <= 1e-5
    for k in g.files:
        if k.startswith("self32/"):
            assert float(g[k]) < 1e-5, k


# ---------------------------------------------------------------------------------------------------------- restatements vs recordings
def test_gradcam_grad_restatement_matches_recorded_conv3_map(golden_dir):
    g = load(golden_dir, "r2p1d_a")
    _, _, H, W = (int(v) for v in g["shape"])
    wts, raw, maps = gradcam_grad_ref(g["act/conv3"], g["grad/conv3"], H, W)
    assert rel_max(wts, g["alpha"]) <= 1e-5
    assert rel_max(raw, g["cam_raw"]) <= 1e-5
    assert float(np.max(np.abs(maps - g["map"]))) <= 1e-5


@pytest.mark.parametrize("name", ["slow", "fast"])
def test_gradcam_grad_restatement_matches_recorded_slowfast_maps(golden_dir, name):
    g = load(golden_dir, "slowfast")
    S = int(g["shape"][2])
    wts, raw, maps = gradcam_grad_ref(g["act/" + name], g["grad/" + name], S, S)
    assert rel_max(wts, g["alpha/" + name]) <= 1e-5
    assert rel_max(raw, g["cam_raw/" + name]) <= 1e-5
    assert float(np.max(np.abs(maps - recorded_map(g["map/" + name])))) <= 1e-5


def test_gradcam_grad_restatement_constant_map_gives_zeros():
    act = np.ones((1, 4, 2, 3, 3)); dact = -np.ones((1, 4, 2, 3, 3))          # negative weights: ReLU leaves an all-zero map
    _, raw, maps = gradcam_grad_ref(act, dact, 6, 6)
    assert not raw.any() and not maps.any()


def test_saliency_map_restatement(golden_dir):
    g = load(golden_dir, "r2p1d_a")
    dx = g["dx"]
    for mode in ("max", "sum"):
        m = saliency_map_ref(dx, mode)
        assert m.shape == (dx.shape[0],) + dx.shape[2:]
        for b in range(dx.shape[0]):
            assert m[b].min() == 0.0 and m[b].max() == 1.0
        # against torch's own reductions of the recorded gradient
        t = torch.from_numpy(dx).double().abs()
        t = t.amax(1) if mode == "max" else t.sum(1)
        lo = t.amin(dim=(1, 2, 3), keepdim=True); hi = t.amax(dim=(1, 2, 3), keepdim=True)
        assert float(np.max(np.abs(m - ((t - lo) / (hi - lo)).numpy()))) <= 1e-12
    assert not saliency_map_ref(np.full((1, 3, 2, 4, 4), -2.5)).any()          # a constant clip gives zeros


# ---------------------------------------------------------------------------------------------------------- ABI and constructors
def test_new_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mi355x_disrupt.h")).read()
    declared = set(re.findall(r"\b(md_[a-z0-9_]+)\s*\(", hdr))
    lib = _native.lib()
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in the header"
        assert name in _native.SIGNATURES, f"{name} has no ctypes prototype"
        assert hasattr(lib, name), f"{name} is not exported by the library"


def test_eval_backward_entry_points_reject_bad_arguments_without_a_gpu():
    import ctypes as C
    lib = _native.lib()
    assert lib.md_bn_eval_bwd(None, None, 10, 4, None, None) == -5                     # MD_ERR_NULL
    assert lib.md_residual_eval_bwd(None, None, None, None, 0.01, 10, 4, None, None, 0, None) == -5
    assert lib.md_saliency_map(None, 1, 3, 2, 4, 4, 0, None, None, None) == -5
    assert lib.md_saliency_scratch_floats(2) > 0 and lib.md_gradcam_grad_scratch_floats(2, 64) > 0
    stem = _native.MdConvDesc(2, 8, 48, 40, 3, 8, 24, 20, 45, 1, 7, 7, 1, 2, 2, 0, 3, 3)
    assert lib.md_stem_dgrad_supported(C.byref(stem)) == 1
    temporal = _native.MdConvDesc(2, 8, 24, 20, 45, 8, 24, 20, 32, 3, 1, 1, 1, 1, 1, 1, 0, 0)
    assert lib.md_stem_dgrad_supported(C.byref(temporal)) == 0
    ls = (C.c_int32 * 4)(1, 1, 1, 1)
    h = C.c_void_p()
    assert lib.md_plan_create(2, 8, 48, 40, ls, 0.01, C.byref(h)) == 0
    assert lib.md_plan_input_grad(h, None, None, None, -1, None, None, None) == -5
    lib.md_plan_destroy(h)


def test_visualisation_constructors():
    from src.models.R2Plus1D import R2Plus1DClassifier
    from src.visualization.visualize_cam import GradCAM_R2Plus1D
    from src.visualization.visualize_saliency import InputGradient
    m = R2Plus1DClassifier(input_size=(3, 8, 48, 40), num_classes=2, layer_sizes=[1, 1, 1, 1], alpha=0.01)
    cam = GradCAM_R2Plus1D(m)
    assert cam.layer == "conv5" and not m.training
    assert GradCAM_R2Plus1D(m, layer="conv3").layer == "conv3"
    with pytest.raises(ValueError):
        GradCAM_R2Plus1D(m, layer="conv6")
    sal = InputGradient(m)
    with pytest.raises(ValueError):
        sal.compute(torch.zeros(1, 3, 8, 48, 40), mode="median")
    with pytest.raises(RuntimeError):
        sal.compute(torch.zeros(1, 3, 8, 48, 40))              # a CPU clip: the path runs on the GPU only
