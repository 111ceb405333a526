#!/usr/bin/env python3
"""Generate the eval-mode backward fixtures (sal_*.npz) in this directory from the REFERENCE implementation.

Run in the build container only (needs the reference checkout; never on the GPU box):

    python tests/golden/make_saliency_golden.py

As in make_xai_golden.py the reference is imported unmodified, with empty stand-ins in ``sys.modules`` for modules that play no
part in the arithmetic.  Every model is put in eval mode and run twice, in fp32 and in fp64; the score is ``logit[:, 0].sum()``
and ``x.grad`` is what ``score.backward()`` leaves.  The fp64 run is what is recorded (stored as float32: 6e-8 relative, far
below every bar a test applies to it); the fp32 run only yields ``self32/<name>`` = max|fp32 - fp64| / max|fp64|, the
reference's distance to itself, which must be below 1e-5 here -- a larger figure means a LeakyReLU / ReLU input changed sign
between the two runs and the fixture could not carry a plain tolerance.

  sal_r2p1d_a    R2Plus1DClassifier([1,1,1,1]), slope 0.01, synth_state seed 1201, clip(2, 8, 48, 40, 1201): logits, input
                 gradient, activation and gradient at res2plus1d.conv3 (forward hook + full backward hook) and the conv3 Grad-CAM
                 channel weights / raw map / map restated as make_xai_golden.cam_map does, per clip.
  sal_r2p1d_lin  the same with slope 1.0 (every LeakyReLU is the identity: the eval-mode trunk is linear); logits and input gradient.
  sal_slowfast   SlowFast(layers [1,1,1,1], alpha 4, tau_fast 1) at slowfast_fixture()'s configuration (T 8, 64 x 64, seed 41, one
                 clip), with hooks on encoder.slownet.layer4[0].downsample[0] (the Conv3d, before its BatchNorm) and
                 encoder.fastnet.l_layer3: both activations, both gradients, both maps, logits and the input gradient.
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

from oracle import r2plus1d as orc                  # noqa: E402
from oracle import slowfast as osf                  # noqa: E402
from src.models.R2Plus1D import R2Plus1DClassifier  # noqa: E402  (reference)
from src.models.slowfast import SlowFast            # noqa: E402  (reference)

torch.set_num_threads(8)


def clip(B, T, H, W, seed):
    """make_xai_golden.clip: uniform integers in [0, 255] minus the BGR means."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, size=(B, 3, T, H, W)).astype("float32")
    x -= np.array([90.0, 98.0, 102.0], dtype="float32").reshape(1, 3, 1, 1, 1)
    return torch.from_numpy(x)


def cam_map(act, grad, H, W):
    """make_xai_golden.cam_map for one clip: act, grad (1, C, T', h, w) -> alpha (1, C), raw (1, T', h, w), map (H, W)."""
    C = act.shape[1]
    alpha = grad.mean(2).reshape(1, C, -1).mean(2)
    raw = torch.relu((alpha.reshape(1, C, 1, 1, 1) * act).sum(1))
    frames = torch.nn.functional.interpolate(raw.permute(1, 0, 2, 3), size=(H, W), mode="bilinear", align_corners=False)
    m = frames.mean(0)[0]
    lo, hi = m.min(), m.max()
    return alpha, raw, (m - lo) / (hi - lo)


def run(model, x, hooked, dtype):
    """Eval-mode forward + backward of logit[:, 0].sum() in `dtype`: logits, x.grad and (activation, gradient) per hooked module."""
    model = model.to(dtype).eval()
    acts, grads, handles = {}, {}, []
    for name, mod in hooked.items():
        handles.append(mod.register_forward_hook(lambda m, i, o, name=name: acts.__setitem__(name, o.detach())))
        handles.append(mod.register_full_backward_hook(lambda m, gi, go, name=name: grads.__setitem__(name, go[0].detach())))
    xx = x.to(dtype).clone().requires_grad_(True)
    logits = model(xx)
    logits[:, 0].sum().backward()
    for h in handles:
        h.remove()
    out = {"logits": logits.detach(), "dx": xx.grad.detach()}
    for name in hooked:
        out["act/" + name] = acts[name]
        out["grad/" + name] = grads[name]
    return out


def both(make_model, x, hooked_of):
    m = make_model()
    r32 = run(m, x, hooked_of(m), torch.float32)
    m = make_model()
    r64 = run(m, x, hooked_of(m), torch.float64)
    rec = {}
    for k, v in r64.items():
        self32 = float((r32[k].double() - v).abs().max() / v.abs().max())
        assert self32 < 1e-5, (k, self32)
        rec[k] = v.numpy().astype(np.float32)
        rec["self32/" + k] = np.float64(self32)
    return rec, r64


def r2p1d_fixture(tag, slope, with_conv3):
    ls, seed, (B, T, H, W) = [1, 1, 1, 1], 1201, (2, 8, 48, 40)

    def make():
        model = R2Plus1DClassifier(input_size=(3, T, H, W), num_classes=2, layer_sizes=ls, alpha=slope)
        params, bufs = orc.synth_state(ls, seed, slope)
        sd = dict(params); sd.update(bufs)
        missing, unexpected = model.load_state_dict(sd, strict=True)
        assert not missing and not unexpected
        return model

    rec, r64 = both(make, clip(B, T, H, W, seed), (lambda m: {"conv3": m.res2plus1d.conv3}) if with_conv3 else (lambda m: {}))
    if with_conv3:
        al, raws, maps = [], [], []
        for b in range(B):
            a, raw, mp = cam_map(r64["act/conv3"][b:b + 1], r64["grad/conv3"][b:b + 1], H, W)
            al.append(a[0].numpy()); raws.append(raw[0].numpy()); maps.append(mp.numpy())
        rec.update(alpha=np.stack(al).astype(np.float32), cam_raw=np.stack(raws).astype(np.float32), map=np.stack(maps).astype(np.float32))
    rec.update(seed=np.int64(seed), shape=np.array([B, T, H, W]), slope=np.float32(slope), layer_sizes=np.array(ls))
    np.savez_compressed(os.path.join(HERE, "sal_%s.npz" % tag), **rec)
    print(tag, {k: float(v) for k, v in rec.items() if k.startswith("self32/")})


def slowfast_fixture():
    layers, T, S, B, seed = [1, 1, 1, 1], 8, 64, 1, 41

    def make():
        m = SlowFast(input_shape=(3, T, S, S), layers=layers, alpha=4, tau_fast=1, num_classes=2, alpha_elu=1.0)
        m.load_state_dict(osf.synth_state({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed), strict=True)
        return m

    hooked = lambda m: {"slow": m.encoder.slownet.layer4[0].downsample[0], "fast": m.encoder.fastnet.l_layer3}
    rec, r64 = both(make, osf.synth_clip(B, T, S, seed + 1), hooked)
    for name in ("slow", "fast"):
        a, raw, mp = cam_map(r64["act/" + name], r64["grad/" + name], S, S)
        rec["alpha/" + name] = a.numpy().astype(np.float32)
        rec["cam_raw/" + name] = raw.numpy().astype(np.float32)
        rec["map/" + name] = mp.numpy().astype(np.float32)[None]
    rec.update(seed=np.int64(seed), shape=np.array([B, T, S, S]), layers=np.array(layers))
    np.savez_compressed(os.path.join(HERE, "sal_slowfast.npz"), **rec)
    print("slowfast", {k: float(v) for k, v in rec.items() if k.startswith("self32/")},
          {k: v.shape for k, v in rec.items() if "/" in k and not k.startswith("self32")})


if __name__ == "__main__":
    r2p1d_fixture("r2p1d_a", 0.01, True)
    r2p1d_fixture("r2p1d_lin", 1.0, False)
    slowfast_fixture()
    for f in sorted(os.listdir(HERE)):
        if f.startswith("sal_"):
            print(f, os.path.getsize(os.path.join(HERE, f)))
