"""GPU tests of the explainability kernels (csrc/xai.hip) and of src.visualization against the reference fixtures
(tests/golden/xai_*.npz) and float64 restatements (tests/test_xai_cpu.py)."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import r2plus1d as orc
from tests.test_xai_cpu import discard, rollout

DEV = torch.device("cuda:0")
VIVIT = dict(patch_size=8, n_classes=2, dim=32, depth=2, n_heads=2, pool="cls", in_channels=3, d_head=16, dropout=0.0,
             embedd_dropout=0.0, scale_dim=2, alpha=0.7)
ROLL = {"roll17": (32, 5), "roll65": (64, 3)}


def _load(golden_dir, tag):
    return np.load(os.path.join(golden_dir, "xai_%s.npz" % tag))


def clip(B, T, H, W, seed):
    """make_xai_golden.py::clip."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, size=(B, 3, T, H, W)).astype("float32")
    x -= np.array([90.0, 98.0, 102.0], dtype="float32").reshape(1, 3, 1, 1, 1)
    return torch.from_numpy(x)


def r2p1d(ls, T, H, W, seed, alpha=0.01):
    from src.models.R2Plus1D import R2Plus1DClassifier
    m = R2Plus1DClassifier(input_size=(3, T, H, W), num_classes=2, layer_sizes=ls, alpha=alpha)
    params, bufs = orc.synth_state(ls, seed, alpha)
    sd = dict(params); sd.update(bufs)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).eval()


class exact_fp32:
    def __enter__(self):
        from src import ops
        ops.set_exact_fp32(True)

    def __exit__(self, *a):
        from src import ops
        ops.set_exact_fp32(False)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["cam_a", "cam_b"])
def test_gradcam_matches_reference_fixture(golden_dir, tag):
    from src.visualization import _xai
    from src.visualization.visualize_cam import GradCAM_R2Plus1D
    g = _load(golden_dir, tag)
    T, H, W = (int(v) for v in g["shape"])
    m = r2p1d([1, 1, 1, 1], T, H, W, int(g["seed"]), float(g["slope"]))
    cam = GradCAM_R2Plus1D(m)
    x = clip(1, T, H, W, int(g["seed"])).to(DEV)
    with exact_fp32():
        maps, logits = cam.compute(x, 0)
        raw = cam.cam_raw.clone()
        with torch.no_grad():
            feat = m.res2plus1d(x)
            h = m.linear
            dfeat = _xai.head_eval_dfeat(feat, h[0], h[1], h[3], float(h[2].alpha), 0)
        torch.cuda.synchronize()
    assert np.max(np.abs(logits.cpu().numpy() - g["logits"])) <= 1e-4 * max(1.0, np.max(np.abs(g["logits"])))
    alpha = dfeat.cpu().numpy() / np.prod(g["act"].shape[2:])
    assert np.max(np.abs(alpha - g["alpha"])) <= 1e-4 * np.max(np.abs(g["alpha"]))
    assert raw.shape == g["cam_raw"].shape
    assert np.max(np.abs(raw.cpu().numpy() - g["cam_raw"])) <= 1e-3 * np.max(np.abs(g["cam_raw"]))
    assert maps.shape == (1, H, W) and np.max(np.abs(maps[0].cpu().numpy() - g["map"])) <= 1e-3
    img, heat, res, fig = cam(x.cpu().to(DEV))
    assert img.shape == (H, W, 3) and heat.shape == (H, W, 3) and heat.dtype == np.uint8 and res.dtype == np.uint8
    if fig is not None:
        import matplotlib.pyplot as plt
        plt.close(fig)


@pytest.mark.gpu
def test_gradcam_batch_equals_single_clips():
    from src.visualization.visualize_cam import GradCAM_R2Plus1D
    m = r2p1d([1, 1, 1, 1], 8, 64, 48, 1201)
    cam = GradCAM_R2Plus1D(m)
    x = clip(3, 8, 64, 48, 1202).to(DEV)
    tgt = torch.tensor([0, 1, 0], device=DEV)
    maps, logits = cam.compute(x, tgt)
    raw = cam.cam_raw.clone()
    for b in range(3):
        mb, lb = cam.compute(x[b:b + 1].contiguous(), int(tgt[b]))
        assert float((mb[0] - maps[b]).abs().max()) <= 1e-5
        assert float((cam.cam_raw[0] - raw[b]).abs().max()) <= 1e-5 * max(1e-6, float(raw[b].abs().max()))
        assert float((lb[0] - logits[b]).abs().max()) <= 1e-5 * max(1.0, float(logits[b].abs().max()))
    assert float(maps.min()) >= 0.0 and float(maps.max()) <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("act", ["elu1", "elu07", "leaky"])
@pytest.mark.parametrize("form", ["fused", "composed"])
def test_head_eval_dfeat_matches_autograd(act, form):
    from src.models._unit import head_apply
    from src.visualization import _xai
    B, D, Hd, K = (4, 128, 64, 2) if form == "fused" else (32, 512, 256, 3)
    alpha = {"elu1": 1.0, "elu07": 0.7, "leaky": -0.01}[act]
    torch.manual_seed(7)
    lin0, bn, lin1 = nn.Linear(D, Hd), nn.BatchNorm1d(Hd), nn.Linear(Hd, K)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5); bn.bias.normal_(0, 0.3)
        bn.running_mean.normal_(0, 0.5); bn.running_var.uniform_(0.5, 2.0)
    ref = nn.Sequential(lin0, bn, nn.ELU(alpha) if alpha >= 0 else nn.LeakyReLU(-alpha), lin1).double().eval()
    feat = torch.randn(B, D, dtype=torch.float64)
    tgt = torch.randint(0, K, (B,))
    f = feat.clone().requires_grad_(True)
    ref(f)[torch.arange(B), tgt].sum().backward()
    with torch.no_grad():
        ref_logits = ref(feat)
    lin0g, bng, lin1g = [copy.deepcopy(mod).float().to(DEV) for mod in (lin0, bn, lin1)]
    fg = feat.float().to(DEV)
    with torch.no_grad():
        logits = head_apply(fg, lin0g, bng, lin1g, alpha, False)
    assert float((logits.cpu().double() - ref_logits).abs().max()) <= 1e-3 * max(1.0, float(ref_logits.abs().max()))
    dfeat = _xai.head_eval_dfeat(fg, lin0g, bng, lin1g, alpha, tgt.to(DEV)).cpu().double()
    assert float((dfeat - f.grad).abs().max()) <= 1e-4 * float(f.grad.abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["mean", "max", "min"])
@pytest.mark.parametrize("S,B,H,dh,bf", [(197, 4, 3, 64, True), (22, 2, 3, 64, True), (17, 5, 2, 16, False)])
def test_attention_probs_fused_matches_fp64(how, S, B, H, dh, bf):
    from src.visualization import _xai
    torch.manual_seed(S + B)
    D = H * dh
    qkv = torch.randn((B, S, 3 * D) if bf else (S, B, 3 * D)) * 1.5
    out = _xai.attention_probs_fused(qkv.to(DEV), H, how, bf).cpu().double()
    q64 = qkv.double() if bf else qkv.double().transpose(0, 1)
    q, k, _ = q64.chunk(3, -1)
    q = q.reshape(B, S, H, dh).transpose(1, 2); k = k.reshape(B, S, H, dh).transpose(1, 2)
    p = torch.softmax(q @ k.transpose(-1, -2) * dh ** -0.5, -1)
    ref = p.mean(1) if how == "mean" else (p.max(1)[0] if how == "max" else p.min(1)[0])
    assert float((out - ref).abs().max()) <= 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["roll17", "roll65"])
@pytest.mark.parametrize("transformer", ["space", "temporal"])
@pytest.mark.parametrize("how", ["mean", "max", "min"])
def test_rollout_kernels_reproduce_fixture_masks(golden_dir, tag, transformer, how):
    from src.visualization.visualize_attention import rollout_from_fused
    g = _load(golden_dir, tag)
    key = "%s/%s/" % (transformer, how)
    fused = torch.from_numpy(g[key + "fused"]).to(DEV)
    disc, _, mask = rollout_from_fused(fused, 1, float(g["discard_ratio"]), 0 if transformer == "space" else 1)
    disc = disc.cpu().numpy()
    assert np.array_equal(disc[:, 0], g[key + "first_after"])                  # the same discard set, values untouched
    assert np.array_equal(disc[:, 1:], g[key + "fused"][:, 1:])
    ref = g[key + "mask"]
    assert np.max(np.abs(mask.cpu().numpy().reshape(ref.shape) - ref)) <= 1e-5 * np.max(np.abs(ref))


def _vivit_from_fixture(g, tag):
    from src.models.ViViT import ViViT
    image, n_frames = ROLL[tag]
    m = ViViT(image_size=image, n_frames=n_frames, **VIVIT)
    m.load_state_dict({k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd/")}, strict=True)
    return m.to(DEV).eval()


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["roll17", "roll65"])
@pytest.mark.parametrize("transformer", ["space", "temporal"])
@pytest.mark.parametrize("how", ["mean", "max", "min"])
def test_rollout_end_to_end_matches_reference_fixture(golden_dir, tag, transformer, how):
    from src.visualization.visualize_attention import ViViTAttentionRollout
    g = _load(golden_dir, tag)
    m = _vivit_from_fixture(g, tag)
    ro = ViViTAttentionRollout(m, head_fusion=how, discard_ratio=float(g["discard_ratio"]), transformer=transformer)
    x = torch.from_numpy(g["x"]).to(DEV)
    with exact_fp32():
        mask = ro(x)
        torch.cuda.synchronize()
    ref = g["%s/%s/mask" % (transformer, how)]
    assert mask.shape == ref.shape
    assert np.max(np.abs(mask - ref)) <= 1e-4 * np.max(np.abs(ref))
    # a batch of two clips: a leading clip axis, each clip as on its own
    with exact_fp32():
        mask2 = ro(torch.cat([x, x], 0))
    assert mask2.shape == (2,) + ref.shape and np.max(np.abs(mask2[0] - mask)) <= 1e-5


@pytest.mark.gpu
def test_rollout_cfg3_matches_fp64_restatement_and_leaves_forward_untouched():
    from src.models.ViViT import ViViT
    from src.visualization.visualize_attention import ViViTAttentionRollout
    torch.manual_seed(3)
    m = ViViT(image_size=224, patch_size=16, n_frames=21, n_classes=2, dim=192, depth=4, n_heads=3, d_head=64).to(DEV).eval()
    x = torch.randn(2, 21, 3, 224, 224, device=DEV)
    with torch.no_grad():
        before = m(x).clone()
    ro = ViViTAttentionRollout(m, head_fusion="mean", discard_ratio=0.9, transformer="space")
    mask = ro(x)
    assert mask.shape == (2, 21, 14, 14)
    fused = ro._buf.cpu().numpy()
    assert fused.shape == (4, 42, 197, 197)
    _, _, ref = rollout(fused, 2, 0.9, 0)
    assert np.max(np.abs(mask - ref.reshape(mask.shape))) <= 1e-5
    # the discard set from the kernels equals the restatement's
    from src.visualization.visualize_attention import rollout_from_fused
    disc, _, _ = rollout_from_fused(ro._buf, 2, 0.9, 0)
    d_ref = discard(fused[:1].reshape(2, 21, 197, 197), 21, int(197 * 197 * 0.9))
    got = disc[0].cpu().numpy().reshape(2, 21, 197, 197)
    assert np.array_equal(got[:, 0] == 0, d_ref[:, 0] == 0)
    del ro, disc
    with torch.no_grad():
        after = m(x)
    assert torch.equal(before, after)
    assert all(getattr(mod, "_xai_recorder", None) is None for mod in m.modules())


@pytest.mark.gpu
def test_eval_mode_backward_guards_still_raise():
    from src.models._unit import HeadFunction
    m = r2p1d([1, 1, 1, 1], 8, 32, 32, 1301)
    x = clip(2, 8, 32, 32, 1302).to(DEV)
    with pytest.raises(RuntimeError, match="eval-mode forward"):
        m.res2plus1d(x).sum().backward()
    with pytest.raises(RuntimeError, match="eval-mode"):
        m(x).sum().backward()
    f = torch.randn(2, 128, device=DEV, requires_grad=True)
    h = m.linear
    out = HeadFunction.apply(f, h[0].weight, h[0].bias, h[1].weight, h[1].bias, h[3].weight, h[3].bias, h[1].running_mean,
                             h[1].running_var, 1.0, 1e-5, 0.1, False)
    with pytest.raises(RuntimeError, match="eval-mode"):
        out.sum().backward()
