"""CPU tests of the explainability tools (src/visualization): float64 restatements of the Grad-CAM map step and of attention
rollout (discard quirk included) reproduce the reference fixtures (tests/golden/xai_*.npz, made by make_xai_golden.py), the JET
table, and the argument checks of the md_head_eval_dfeat / md_gradcam / md_attention_probs_fused / md_rollout_* entry points."""
import ctypes as C
import os

import numpy as np
import pytest

from src import _native
from src.visualization import visualize_attention as va
from src.visualization import visualize_cam as vc


def _load(golden_dir, tag):
    return np.load(os.path.join(golden_dir, "xai_%s.npz" % tag))


def resize_bilinear(img, OH, OW):
    """(h, w) -> (OH, OW), float64, F.interpolate(mode='bilinear', align_corners=False)."""
    h, w = img.shape

    def axis(n_in, n_out):
        s = np.maximum((np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5, 0.0)
        i0 = np.floor(s).astype(int)
        i1 = np.minimum(i0 + 1, n_in - 1)
        return i0, i1, s - i0

    y0, y1, ly = axis(h, OH)
    x0, x1, lx = axis(w, OW)
    ly, lx = ly[:, None], lx[None, :]
    top = img[y0][:, x0] * (1 - lx) + img[y0][:, x1] * lx
    bot = img[y1][:, x0] * (1 - lx) + img[y1][:, x1] * lx
    return top * (1 - ly) + bot * ly


def gradcam_map(act, dfeat_or_grad, H, W, from_grad=True):
    """act (B, C, T', h, w); the channel weights from the conv5 gradient (B, C, T', h, w) or from dfeat (B, C).  Returns alpha, the
    ReLU'd map (B, T', h, w) and the normalised (B, H, W) map, a constant map giving zeros."""
    act = np.asarray(act, np.float64)
    B, Cc, Tq, h, w = act.shape
    g = np.asarray(dfeat_or_grad, np.float64)
    alpha = g.reshape(B, Cc, -1).mean(-1) if from_grad else g / (Tq * h * w)
    raw = np.maximum(np.einsum("bc,bcthw->bthw", alpha, act), 0.0)
    out = np.zeros((B, H, W))
    for b in range(B):
        m = np.mean([resize_bilinear(raw[b, t], H, W) for t in range(Tq)], axis=0)
        lo, hi = m.min(), m.max()
        out[b] = (m - lo) / (hi - lo) if hi > lo else 0.0
    return alpha, raw, out


def discard(fused, n_seq_per_clip, k):
    """The reference's discard step per clip: each sequence's k smallest flat entries (ties: lowest index first), index 0
    excepted, zeroed in the clip's first sequence only."""
    out = np.array(fused, np.float64, copy=True)
    L_shape = out.shape
    S = L_shape[-1]
    flat = out.reshape(-1, n_seq_per_clip, S * S)
    src = np.asarray(fused).reshape(-1, n_seq_per_clip, S * S)
    for c in range(flat.shape[0]):
        for s in range(n_seq_per_clip):
            idx = np.argsort(src[c, s], kind="stable")[:k]
            idx = idx[idx != 0]
            flat[c, 0, idx] = 0.0
    return flat.reshape(L_shape)


def rollout(fused_layers, n_clips, ratio, kind):
    """float64 rollout of (L, n_seq, S, S) head-fused maps: (discarded maps, chain product, per-clip normalised mask)."""
    f = np.asarray(fused_layers, np.float64)
    L, nseq, S, _ = f.shape
    nspc = nseq // n_clips
    d = discard(f.reshape(L * n_clips, nspc, S, S), nspc, int(S * S * ratio)).reshape(L, nseq, S, S)
    eye = np.eye(S)
    res = np.broadcast_to(eye, (nseq, S, S)).copy()
    for l in range(L):
        res = np.matmul((d[l] + eye) / 2.0, res)
    if kind == 0:
        m = res[:, 0, 1:].reshape(n_clips, nspc, S - 1)
    else:
        m = res[:, 1:, 1:].reshape(n_clips, nspc, S - 1, S - 1)
    m = m / m.reshape(n_clips, -1).max(-1).reshape((n_clips,) + (1,) * (m.ndim - 1))
    return d, res, m


@pytest.mark.parametrize("tag", ["cam_a", "cam_b"])
def test_gradcam_map_restatement_matches_reference_fixture(golden_dir, tag):
    g = _load(golden_dir, tag)
    T, H, W = (int(v) for v in g["shape"])
    alpha, raw, out = gradcam_map(g["act"], g["grad"], H, W)
    assert np.allclose(alpha, g["alpha"], rtol=1e-5, atol=1e-9)
    assert np.max(np.abs(raw - g["cam_raw"])) <= 1e-5 * np.max(np.abs(g["cam_raw"]))
    assert out.shape == (1, H, W) and np.max(np.abs(out[0] - g["map"])) <= 1e-5
    # the gradient at conv5 is dfeat / (T'*h*w) everywhere (the pool is the only op after it): the shortcut the kernels take
    grad = g["grad"].astype(np.float64)
    assert np.allclose(grad, grad.reshape(1, grad.shape[1], -1)[..., :1, None, None], rtol=1e-5, atol=0)
    dfeat = grad.reshape(1, grad.shape[1], -1)[..., 0] * np.prod(grad.shape[2:])
    a2, _, out2 = gradcam_map(g["act"], dfeat, H, W, from_grad=False)
    assert np.allclose(a2, alpha, rtol=1e-5, atol=1e-9) and np.max(np.abs(out2 - out)) <= 1e-6


def test_gradcam_constant_map_gives_zeros():
    _, raw, out = gradcam_map(-np.ones((1, 4, 2, 3, 3)), np.ones((1, 4)), 12, 12, from_grad=False)
    assert np.all(raw == 0) and np.all(out == 0)


@pytest.mark.parametrize("tag", ["roll17", "roll65"])
@pytest.mark.parametrize("transformer", ["space", "temporal"])
@pytest.mark.parametrize("how", ["mean", "max", "min"])
def test_rollout_restatement_matches_reference_fixture(golden_dir, tag, transformer, how):
    g = _load(golden_dir, tag)
    key = "%s/%s/" % (transformer, how)
    fused = g[key + "fused"]
    d, _, m = rollout(fused, 1, float(g["discard_ratio"]), 0 if transformer == "space" else 1)
    assert np.array_equal(d[:, 0], g[key + "first_after"].astype(np.float64))
    assert np.array_equal(d[:, 1:], fused[:, 1:].astype(np.float64))          # only the first sequence is changed (quirk kept)
    ref = g[key + "mask"]
    assert np.max(np.abs(m.reshape(ref.shape) - ref)) <= 1e-5 * np.max(np.abs(ref))


def test_discard_takes_exactly_k_with_ties_by_index():
    S = 4
    f = np.full((1, 1, S, S), 0.5)
    f[0, 0, 0, 3] = 0.1
    d = discard(f, 1, 5)
    zeroed = np.flatnonzero(d.reshape(-1) == 0)
    assert list(zeroed) == [1, 2, 3, 4]       # 3 (smallest), then the ties 0, 1, 2, 4 (lowest index first); index 0 kept


def test_jet_table_is_monotone_in_bgr_order():
    t = vc.JET_BGR.astype(int)
    assert t.shape == (256, 3) and vc.JET_BGR.dtype == np.uint8
    dom = t.argmax(1)
    assert dom[0] == 0 and dom[-1] == 2 and np.all(np.diff(dom) >= 0)        # blue -> green -> red
    b, g, r = t[:, 0], t[:, 1], t[:, 2]
    assert np.all(np.diff(r[: np.argmax(r) + 1]) >= 0) and np.all(np.diff(r[np.argmax(r):]) <= 0)
    assert np.all(np.diff(b[: np.argmax(b) + 1]) >= 0) and np.all(np.diff(b[np.argmax(b):]) <= 0)
    assert np.argmax(b) < np.argmax(g) < np.argmax(r)
    img = vc.apply_color_map_jet(np.array([[0, 255]], np.uint8))
    assert img.shape == (1, 2, 3) and tuple(img[0, 0]) == tuple(vc.JET_BGR[0])


def test_unknown_head_fusion_raises_value_error():
    with pytest.raises(ValueError):
        va.ViViTAttentionRollout(object(), head_fusion="median")


def test_xai_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _native.lib()
    p = C.c_void_p(256)                 # never dereferenced: every check below returns before any HIP call
    # md_head_eval_dfeat
    args = [p, 2, 8, 4, 2] + [p] * 6 + [1e-5, 1.0, p, p, p, None]
    bad = list(args); bad[0] = None
    assert lib.md_head_eval_dfeat(*bad) == -5
    bad = list(args); bad[14] = None
    assert lib.md_head_eval_dfeat(*bad) == -5
    bad = list(args); bad[1] = 0
    assert lib.md_head_eval_dfeat(*bad) == -1
    bad = list(args); bad[2] = 20000
    assert lib.md_head_eval_dfeat(*bad) == -2
    # md_gradcam(act, rows_per_clip, C, Cpad, T', h, w, dfeat, B, OH, OW, cam_raw, out)
    g = [p, 3 * 8 * 8, 128, 128, 3, 8, 8, p, 2, 128, 128, p, p, None]
    bad = list(g); bad[12] = None
    assert lib.md_gradcam(*bad) == -5
    bad = list(g); bad[1] = 100                       # rows per clip != T'*h*w
    assert lib.md_gradcam(*bad) == -1
    bad = list(g); bad[3] = 64                        # Cpad < C
    assert lib.md_gradcam(*bad) == -1
    bad = list(g); bad[9] = 0
    assert lib.md_gradcam(*bad) == -1
    bad = list(g); bad[4], bad[1] = 300, 300 * 64     # map of one clip larger than LDS
    assert lib.md_gradcam(*bad) == -2
    # md_attention_probs_fused(qkv, S, B, D, H, batch_first, fusion, out)
    a = [p, 197, 2, 192, 3, 1, 0, p, None]
    bad = list(a); bad[0] = None
    assert lib.md_attention_probs_fused(*bad) == -5
    bad = list(a); bad[6] = 3                         # fusion enum
    assert lib.md_attention_probs_fused(*bad) == -1
    bad = list(a); bad[5] = 2                         # batch_first enum
    assert lib.md_attention_probs_fused(*bad) == -1
    bad = list(a); bad[4] = 5                         # D % H != 0
    assert lib.md_attention_probs_fused(*bad) == -1
    bad = list(a); bad[1] = 4000                      # S beyond LDS
    assert lib.md_attention_probs_fused(*bad) == -2
    bad = list(a); bad[0] = C.c_void_p(260)           # not 16-byte aligned
    assert lib.md_attention_probs_fused(*bad) == -2
    # md_rollout_discard(fused, n_seq_per_clip, B_clips, S, k, fused_out)
    d = [p, 21, 2, 197, 34928, C.c_void_p(1 << 40), None]
    bad = list(d); bad[5] = None
    assert lib.md_rollout_discard(*bad) == -5
    bad = list(d); bad[4] = 197 * 197 + 1
    assert lib.md_rollout_discard(*bad) == -1
    bad = list(d); bad[4] = -1
    assert lib.md_rollout_discard(*bad) == -1
    bad = list(d); bad[1] = 0
    assert lib.md_rollout_discard(*bad) == -1
    bad = list(d); bad[5] = C.c_void_p(256 + 4096)    # overlaps the input
    assert lib.md_rollout_discard(*bad) == -2
    # md_rollout_chain(fused_layers, L, n_seq, S, result)
    assert lib.md_rollout_chain(None, 4, 42, 197, p, None) == -5
    assert lib.md_rollout_chain(p, 0, 42, 197, p, None) == -1
    assert lib.md_rollout_chain(p, 4, 42, 5000, p, None) == -2
    # md_rollout_mask(result, B_clips, n_seq_per_clip, S, kind, out)
    assert lib.md_rollout_mask(p, 2, 21, 197, 0, None, None) == -5
    assert lib.md_rollout_mask(p, 2, 21, 197, 2, p, None) == -1
    assert lib.md_rollout_mask(p, 2, 21, 1, 0, p, None) == -1
    assert lib.md_rollout_mask(p, 0, 21, 197, 0, p, None) == -1
