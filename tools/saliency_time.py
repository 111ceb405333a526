#!/usr/bin/env python3
"""Time the eval-mode backward tools on the GPU and print one JSON line (also written to --out): ms per clip of the input
gradient (InputGradient.compute), SmoothGrad n = 8, conv3 Grad-CAM (GradCAM_R2Plus1D(layer="conv3")) for R(2+1)D [1,2,2,1] at the
bench shape (8, 3, 21, 128, 128), and of GradCAM_SlowFast at the cfg5 shape (SlowFast [1,2,2,1], 32 frames, 224 x 224), each next
to the eval forward of the same model and batch measured in the same process.  Every figure is the median over --repeats of a
device-event interval around --iters calls, after a warm-up.  Usage: python tools/saliency_time.py [--iters N] [--repeats R]
[--slowfast-batch B] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "disruption-prediciton-based-on-multimodal-deep-learning_amd")]

import torch  # noqa: E402


def _time(fn, iters, repeats, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / iters)
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--slowfast-batch", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("saliency_time.py measures on the GPU; none is visible")
    from src.models.R2Plus1D import R2Plus1DClassifier
    from src.models.slowfast import SlowFast
    from src.visualization.visualize_cam import GradCAM_R2Plus1D, GradCAM_SlowFast
    from src.visualization.visualize_saliency import InputGradient
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B = 8
    m = R2Plus1DClassifier(input_size=(3, 21, 128, 128), num_classes=2, layer_sizes=[1, 2, 2, 1], alpha=0.01).to(dev).eval()
    x = torch.randn(B, 3, 21, 128, 128, device=dev) * 60.0
    sal, cam3 = InputGradient(m), GradCAM_R2Plus1D(m, layer="conv3")
    gen = torch.Generator(device=dev).manual_seed(1)
    with torch.no_grad():
        fwd = _time(lambda: m(x), a.iters, a.repeats)
    grad = _time(lambda: sal.compute(x, 0), a.iters, a.repeats)
    smooth = _time(lambda: sal.compute(x, 0, smooth=8, sigma=0.1, generator=gen), max(1, a.iters // 4), a.repeats)
    c3 = _time(lambda: cam3.compute(x, 0), a.iters, a.repeats)
    del sal, cam3, m, x
    torch.cuda.empty_cache()
    Bs = a.slowfast_batch
    sf = SlowFast(input_shape=(3, 32, 224, 224), layers=[1, 2, 2, 1], alpha=4, tau_fast=1, num_classes=2).to(dev).eval()
    xs = torch.randn(Bs, 3, 32, 224, 224, device=dev)
    scam = GradCAM_SlowFast(sf)
    with torch.no_grad():
        sf_fwd = _time(lambda: sf(xs), max(1, a.iters // 2), a.repeats)
    sf_cam = _time(lambda: scam.compute(xs, 0), max(1, a.iters // 2), a.repeats)
    line = json.dumps({"metric": "saliency_ms_per_clip",
                       "r2p1d_1221_8x21x128": {"eval_forward": round(fwd / B, 4), "input_gradient": round(grad / B, 4),
                                               "smoothgrad_n8": round(smooth / B, 4), "gradcam_conv3": round(c3 / B, 4), "batch": B},
                       "slowfast_1221_32x224": {"eval_forward": round(sf_fwd / Bs, 4), "gradcam_slowfast": round(sf_cam / Bs, 4),
                                                "batch": Bs},
                       "iters": a.iters, "repeats": a.repeats,
                       "note": "each figure includes its own eval forward; GradCAM_SlowFast synchronises the device once per call"})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
