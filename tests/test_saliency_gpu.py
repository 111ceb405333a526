"""GPU tests of the eval-mode backward: the kernels alone against float64 NumPy / torch, the R(2+1)D trunk against the reference
recordings (tests/golden/sal_*.npz) and, at the headline shape, against the fp64 oracle on the HIP path's activation pattern
(tests/kink_util.py), layer Grad-CAM, SlowFast, SmoothGrad, and the training path after an eval-mode backward."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import r2plus1d as orc
from tests import kink_util as ku
from tests.test_saliency_cpu import clip, gradcam_grad_ref, load, oracle_r2p1d, recorded_map, rel_max, saliency_map_ref, slowfast_state

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BGR = np.array([90.0, 98.0, 102.0], dtype="float32").reshape(1, 3, 1, 1, 1)


class arithmetic:
    """exact-fp32 or the default split-precision convolutions for the duration of a block."""

    def __init__(self, exact):
        self.exact = exact

    def __enter__(self):
        from src import ops
        ops.set_exact_fp32(self.exact)

    def __exit__(self, *a):
        from src import ops
        ops.set_exact_fp32(False)


def r2p1d(ls, T, H, W, seed, alpha=0.01):
    from src.models.R2Plus1D import R2Plus1DClassifier
    m = R2Plus1DClassifier(input_size=(3, T, H, W), num_classes=2, layer_sizes=ls, alpha=alpha)
    params, bufs = orc.synth_state(ls, seed, alpha)
    sd = dict(params); sd.update(bufs)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).eval()


def model_of(g):
    B, T, H, W = (int(v) for v in g["shape"])
    return r2p1d([int(v) for v in g["layer_sizes"]], T, H, W, int(g["seed"]), float(g["slope"])), clip(B, T, H, W, int(g["seed"])).to(DEV)


# ================================================================================================================ kernels alone
def _view(y, scale, shift, slope):
    from src import ops
    return ops.view(y, scale, shift, slope)


def _bn_ref(dA, y, scale, shift, slope, C):
    """fp64 product; the sign from the same fp32 fmaf(scale, y, shift) the kernels evaluate (fp64 of fp32 operands rounded once)."""
    p = (scale.astype(np.float64) * y.astype(np.float64) + shift.astype(np.float64)).astype(np.float32)
    f = np.where(p > 0, 1.0, np.float64(np.float32(slope)))
    out = dA.astype(np.float64) * f * scale.astype(np.float64)
    out[:, C:] = 0.0
    return out, p


def _elem_ok(got, ref, tol=1e-6):
    got = got.astype(np.float64)
    bad = np.abs(got - ref) > tol * np.abs(ref) + 1e-37
    return not bad.any(), float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-30)))


@pytest.mark.parametrize("C_", [3, 16, 45, 64, 72, 128])
@pytest.mark.parametrize("slope", [0.01, 0.0, 1.0])
def test_bn_eval_bwd_kernel(C_, slope):
    from src import _native as N, ops
    rng = np.random.default_rng(100 + C_)
    rows, Cp = 1237, (C_ + 3) & ~3                     # not a multiple of any row tile
    y = rng.standard_normal((rows, Cp)).astype(np.float32)
    dA = rng.standard_normal((rows, Cp)).astype(np.float32)       # pad columns deliberately non-zero: the kernel must write zeros
    scale = np.zeros(Cp, np.float32); shift = np.zeros(Cp, np.float32)
    scale[:C_] = rng.uniform(-1.5, 1.5, C_); shift[:C_] = rng.standard_normal(C_) * 0.3
    ref, _ = _bn_ref(dA, y, scale, shift, slope, C_)
    yg, sg, hg = (torch.from_numpy(a).to(DEV) for a in (y, scale, shift))
    for inplace in (False, True):
        dg = torch.from_numpy(dA).to(DEV)
        out = ops.bn_eval_backward(dg, _view(yg, sg, hg, slope), C_, inplace=inplace)
        torch.cuda.synchronize()
        assert (out.data_ptr() == dg.data_ptr()) == inplace
        got = out.cpu().numpy()
        ok, worst = _elem_ok(got[:, :C_], ref[:, :C_])
        print("bn_eval_bwd C=%d slope=%g inplace=%d worst relative error %.2e" % (C_, slope, inplace, worst))
        assert ok, worst
        assert not got[:, C_:].any()
    # a plain view (no BatchNorm) passes the gradient through
    dg = torch.from_numpy(dA).to(DEV)
    out = ops.bn_eval_backward(dg, _view(yg, None, None, 1.0), C_)
    assert torch.equal(out[:, :C_], dg[:, :C_]) and not out[:, C_:].any()


@pytest.mark.parametrize("C_", [3, 16, 45, 64, 72, 128])
@pytest.mark.parametrize("alpha", [0.01, 0.0, 1.0])
@pytest.mark.parametrize("skip_unit", [False, True])
def test_residual_eval_bwd_kernel(C_, alpha, skip_unit):
    from src import _native as N, ops
    rng = np.random.default_rng(200 + C_)
    rows, Cp = 1013, (C_ + 3) & ~3
    ym, ys, dZ, acc0 = (rng.standard_normal((rows, Cp)).astype(np.float32) for _ in range(4))
    sm = np.zeros(Cp, np.float32); hm = np.zeros(Cp, np.float32); ss = np.zeros(Cp, np.float32); hs = np.zeros(Cp, np.float32)
    sm[:C_] = rng.uniform(-1.5, 1.5, C_); hm[:C_] = rng.standard_normal(C_) * 0.3
    ss[:C_] = rng.uniform(-1.5, 1.5, C_); hs[:C_] = rng.standard_normal(C_) * 0.3
    slope = 0.01
    lk = lambda v, s: np.where(v > 0, v, v * np.float32(s)).astype(np.float32)
    pm = (sm.astype(np.float64) * ym + hm).astype(np.float32)
    a_skip = lk((ss.astype(np.float64) * ys + hs).astype(np.float32), slope) if skip_unit else ys
    z = lk((a_skip + lk(pm, slope)).astype(np.float32), alpha)
    d = dZ.astype(np.float64) * np.where(z > 0, 1.0, np.float64(np.float32(alpha)))
    ref_main = d * np.where(pm > 0, 1.0, np.float64(np.float32(slope))) * sm.astype(np.float64)
    if skip_unit:
        ps = (ss.astype(np.float64) * ys + hs).astype(np.float32)
        ref_s = d * np.where(ps > 0, 1.0, np.float64(np.float32(slope))) * ss.astype(np.float64)
    else:
        ref_s = d.copy()
    ref_main[:, C_:] = 0.0; ref_s[:, C_:] = 0.0
    g = lambda a: torch.from_numpy(a).to(DEV)
    ymg, ysg, zg, smg, hmg, ssg, hsg = (g(a) for a in (ym, ys, z, sm, hm, ss, hs))
    mv = _view(ymg, smg, hmg, slope)
    sv = _view(ysg, ssg, hsg, slope) if skip_unit else None
    L = N.lib()
    for mode in ("out", "inplace", "accumulate"):
        dZg = g(dZ); dmain = torch.empty_like(dZg)
        dS = dZg if mode == "inplace" else (g(acc0) if mode == "accumulate" else torch.empty_like(dZg))
        N.check(L.md_residual_eval_bwd(ops._p(dZg), ops._p(zg), C.byref(mv), None if sv is None else C.byref(sv), alpha, rows, C_,
                                       ops._p(dmain), ops._p(dS), int(mode == "accumulate"), ops._stream()), "md_residual_eval_bwd")
        torch.cuda.synchronize()
        gm, gs = dmain.cpu().numpy(), dS.cpu().numpy()
        ok, worst = _elem_ok(gm[:, :C_], ref_main[:, :C_])
        assert ok, (mode, worst)
        want_s = ref_s if mode != "accumulate" else (acc0.astype(np.float64) + ref_s.astype(np.float32).astype(np.float64))
        if mode == "accumulate":            # one more fp32 rounding, of a sum that may cancel: absolute bound on the scale of the operands
            assert float(np.max(np.abs(gs[:, :C_] - want_s[:, :C_]))) <= 1e-6 * float(np.max(np.abs(want_s)))
        else:
            ok, worst = _elem_ok(gs[:, :C_], want_s[:, :C_])
            assert ok, (mode, worst)
            assert not gs[:, C_:].any()
        assert not gm[:, C_:].any()


@pytest.mark.parametrize("shape", [(2, 8, 48, 40), (1, 3, 33, 27), (1, 2, 128, 128)])
def test_stem_data_gradient(shape):
    """The stem's 1x7x7 / stride-2 data gradient (3 input channels) against torch.nn.grad.conv3d_input in fp64 on the CPU, at the
    tolerance tests/test_conv_random_gpu.py applies to data gradients (5e-5 of the largest element), in both arithmetic modes
    (the dedicated kernel is exact fp32 in either), and the generic md_conv_dgrad path for the same geometry."""
    from src import _native as N, ops
    from tests.test_ops_gpu import cl, uncl, relerr
    Bn, T, H, W = shape
    g = torch.Generator().manual_seed(5)
    w = torch.randn(45, 3, 1, 7, 7, generator=g) / np.sqrt(3 * 49)
    d = ops.make_desc(Bn, T, H, W, 3, 45, (1, 7, 7), (1, 2, 2), (0, 3, 3))
    dy = torch.randn(Bn, 45, d.To, d.Ho, d.Wo, generator=g)
    ref = torch.nn.grad.conv3d_input((Bn, 3, T, H, W), w.double(), dy.double(), (1, 2, 2), (0, 3, 3))
    dyg, wg = cl(dy).to(DEV), w.to(DEV)
    L = N.lib()
    assert L.md_stem_dgrad_supported(C.byref(d)) == 1
    for exact in (False, True):
        with arithmetic(exact):
            out = torch.full((Bn, T, H, W, 4), float("nan"), device=DEV)
            N.check(L.md_stem_dgrad(C.byref(d), ops._p(dyg), ops._p(wg), ops._p(out), ops._stream()), "md_stem_dgrad")
            _, wd = ops.pack_weights(d, wg)
            gen = ops.conv_dgrad(d, dyg, wd)
            torch.cuda.synchronize()
        e, eg = relerr(uncl(out.cpu(), 3), ref), relerr(uncl(gen.cpu(), 3), ref)
        print("stem dgrad %s exact=%d: dedicated %.2e generic %.2e" % (shape, exact, e, eg))
        assert e < 5e-5 and eg < 5e-5
        assert not out[..., 3:].any()


@pytest.mark.parametrize("act", ["elu1", "leaky"])
def test_head_eval_bwd_matches_autograd(act):
    from src.visualization import _xai
    B, D, Hd, K = 4, 128, 64, 3
    alpha = {"elu1": 1.0, "leaky": -0.01}[act]
    torch.manual_seed(11)
    lin0, bn, lin1 = nn.Linear(D, Hd), nn.BatchNorm1d(Hd), nn.Linear(Hd, K)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5); bn.bias.normal_(0, 0.3); bn.running_mean.normal_(0, 0.3); bn.running_var.uniform_(0.5, 1.5)
    bn.eval()
    f = torch.randn(B, D, dtype=torch.float64, requires_grad=True)
    dl = torch.randn(B, K, dtype=torch.float64)
    mods = [m.double() for m in (lin0, bn, lin1)]
    h = mods[1](mods[0](f))
    h = torch.nn.functional.elu(h, alpha) if alpha >= 0 else torch.nn.functional.leaky_relu(h, -alpha)
    ref, = torch.autograd.grad(mods[2](h), f, dl)
    for m in (lin0, bn, lin1):
        m.float().to(DEV)
    got = _xai.head_eval_bwd(f.detach().float().to(DEV), lin0, bn, lin1, alpha, dl.float().to(DEV))
    assert rel_max(got.cpu().numpy(), ref.numpy()) <= 1e-5
    # one-hot dlogits reproduce md_head_eval_dfeat bit for bit (same device code)
    one = torch.zeros(B, K); one[:, 1] = 1.0
    a = _xai.head_eval_bwd(f.detach().float().to(DEV), lin0, bn, lin1, alpha, one.to(DEV))
    b = _xai.head_eval_dfeat(f.detach().float().to(DEV), lin0, bn, lin1, alpha, 1)
    assert torch.equal(a, b)


def test_saliency_map_kernel_matches_restatement():
    from src.visualization import _xai
    rng = np.random.default_rng(3)
    dx = rng.standard_normal((3, 3, 5, 37, 29)).astype(np.float32)
    dx[2] = 0.25                                                   # a constant clip: zeros
    for mode in ("max", "sum"):
        got = _xai.saliency_map(torch.from_numpy(dx).to(DEV), mode)
        again = _xai.saliency_map(torch.from_numpy(dx).to(DEV), mode)
        ref = saliency_map_ref(dx, mode)
        assert float(np.max(np.abs(got.cpu().numpy() - ref))) <= 1e-6
        assert torch.equal(got, again) and not got[2].any()


@pytest.mark.parametrize("geom", [(2, 64, 4, 12, 10, 48, 40), (1, 32, 21, 64, 64, 128, 128)])
def test_gradcam_grad_kernel_matches_restatement(geom):
    """The second geometry (86016 positions per clip) does not fit the LDS: the map kernel samples from memory."""
    from src.visualization import _xai
    from tests.test_ops_gpu import cl
    B, Cc, Tq, h, w, OH, OW = geom
    g = torch.Generator().manual_seed(9)
    act = torch.randn(B, Cc, Tq, h, w, generator=g); dact = torch.randn(B, Cc, Tq, h, w, generator=g) * 1e-3
    rw, rraw, rmap = gradcam_grad_ref(act.numpy(), dact.numpy(), OH, OW)
    a2 = cl(act).reshape(-1, Cc).to(DEV); d2 = cl(dact).reshape(-1, Cc).to(DEV)
    wts, raw, maps = _xai.gradcam_grad(a2, d2, Cc, B, Tq, h, w, OH, OW)
    wts2, raw2, maps2 = _xai.gradcam_grad(a2, d2, Cc, B, Tq, h, w, OH, OW)
    assert torch.equal(maps, maps2) and torch.equal(wts, wts2)
    assert rel_max(wts.cpu().numpy(), rw) <= 1e-4            # a mean of ~1e3..1e5 fp32 terms of either sign
    assert float(np.max(np.abs(raw.cpu().numpy() - rraw))) <= 1e-3 * float(np.max(np.abs(rraw)))
    assert float(np.max(np.abs(maps.cpu().numpy() - rmap))) <= 1e-3


# ================================================================================================================ trunk, kink-free
def eval_preactivations(model, x):
    """kink_util.hip_preactivations for the EVAL-mode forward: every LeakyReLU pre-activation the HIP path used, read out of a
    workspace of its own (md_plan_unit_layout / md_plan_z_layout), by the oracle's names."""
    net = model.res2plus1d
    B, _, T, H, W = x.shape
    plan = net._plan(B, T, H, W)
    units = net.unit_modules()
    ws = plan.new_workspace(x.device)
    plan.forward(x.contiguous().float(), ws, [u.conv.weight for u in units], [u.bn.weight for u in units], [u.bn.bias for u in units],
                 [u.bn.running_mean for u in units], [u.bn.running_var for u in units], False)
    torch.cuda.synchronize()
    names = [u.name for u in orc.all_units(net.layer_sizes, net.alpha)]
    pre = {}
    for i, name in enumerate(names):
        d = plan.descs[i]
        raw, st = plan.unit_tensors(ws, i)
        pre[name] = ku._to_ncthw(torch.addcmul(st[3].view(1, -1), raw, st[2].view(1, -1)), d.Cout, (d.N, d.To, d.Ho, d.Wo)).cpu()
    idx = {n: i for i, n in enumerate(names)}
    for k, bp in enumerate(orc.block_prefixes(net.layer_sizes)):
        z, Cc = plan.z_tensor(ws, 2 + k)
        d = plan.descs[idx[bp + ".conv2.temporal_conv"]]
        zz = ku._to_ncthw(z, Cc, (d.N, d.To, d.Ho, d.Wo)).cpu()
        pre[bp + ".relu"] = torch.where(zz > 0, zz, zz / net.alpha) if net.alpha != 0 else zz
    return pre


def _both_paths(m, x):
    """x.grad through model.eval() + backward(), and through InputGradient.compute."""
    from src.visualization.visualize_saliency import InputGradient
    xa = x.clone().requires_grad_(True)
    logits = m(xa)
    logits[:, 0].sum().backward()
    for p in m.parameters():
        assert p.grad is None                      # the documented deviation: no parameter gradients in eval mode
    grad, maps, lg = InputGradient(m).compute(x, target=0)
    torch.cuda.synchronize()
    return xa.grad.detach(), grad, maps, logits.detach(), lg


@pytest.mark.parametrize("exact", [True, False], ids=["exact_fp32", "split"])
@pytest.mark.parametrize("tag", ["r2p1d_lin", "r2p1d_a"])
def test_trunk_input_gradient_matches_reference_recording(golden_dir, tag, exact):
    g = load(golden_dir, tag)
    m, x = model_of(g)
    with arithmetic(exact):
        dx_auto, dx_tool, maps, logits, lg = _both_paths(m, x)
        pre = eval_preactivations(m, x) if tag == "r2p1d_a" else None
    ref = g["dx"]
    e_auto, e_tool = rel_max(dx_auto.cpu().numpy(), ref), rel_max(dx_tool.cpu().numpy(), ref)
    print("%s %s: max|dx - ref64| / max|ref64|: autograd %.3e, InputGradient %.3e; logits %.3e" % (
        tag, "exact" if exact else "split", e_auto, e_tool, rel_max(logits.cpu().numpy(), g["logits"])))
    if pre is not None:
        tap = {}
        oracle_r2p1d(g, tap=tap)
        fl = ku.flips(pre, tap)
        for name, i, vh, vo, rms in fl[:12]:
            print("  sign flip: %s[%d] hip %+.3e fp64 oracle %+.3e (tensor rms %.3e)" % (name, i, vh, vo, rms))
        if fl:
            # the reference shows none against itself at this shape; with a flip the plain comparison is not meaningful: the fp64
            # oracle on the HIP pattern takes the recording's place
            print("  %d flips: comparing with the fp64 oracle on the HIP activation pattern instead of the recording" % len(fl))
            assert len(fl) <= ku.max_flips(sum(v.numel() for v in pre.values()))
            for name, i, vh, vo, rms in fl:
                assert abs(vh) <= 1e-4 * rms and abs(vo) <= 1e-4 * rms
            _, dxp = oracle_r2p1d(g, force=ku.sign_masks(pre))
            ref = dxp.numpy()
            e_auto, e_tool = rel_max(dx_auto.cpu().numpy(), ref), rel_max(dx_tool.cpu().numpy(), ref)
            print("  on the HIP pattern: autograd %.3e, InputGradient %.3e" % (e_auto, e_tool))
    assert rel_max(logits.cpu().numpy(), g["logits"]) <= 1e-3 and torch.equal(logits, lg)
    assert e_auto <= 1e-3 and e_tool <= 1e-3, (e_auto, e_tool)
    assert torch.equal(dx_auto, dx_tool)           # the same launches on the same bytes
    assert float(np.max(np.abs(maps.cpu().numpy() - saliency_map_ref(dx_tool.cpu().numpy())))) <= 1e-6


# ================================================================================================================ trunk, headline shape
def test_trunk_input_gradient_headline_shape_on_hip_pattern():
    """[1,2,2,1], (2,3,21,128,128), default arithmetic: flips against the fp64 oracle listed, capped by kink_util.max_flips and
    within 1e-4 of their tensor's rms; dx against the fp64 oracle evaluated on the HIP pattern: 1e-3 of its maximum."""
    torch.set_num_threads(16)
    ls, (B, T, H, W), seed, slope = [1, 2, 2, 1], (2, 21, 128, 128), 1101, 0.01
    m = r2p1d(ls, T, H, W, seed, slope)
    x = clip(B, T, H, W, seed)
    xa = x.to(DEV).requires_grad_(True)
    m(xa)[:, 0].sum().backward()
    pre = eval_preactivations(m, x.to(DEV))
    torch.cuda.synchronize()
    g = {"layer_sizes": np.array(ls), "shape": np.array([B, T, H, W]), "seed": seed, "slope": slope}
    tap = {}
    _, dx_own = oracle_r2p1d(g, tap=tap)
    fl = ku.flips(pre, tap)
    total = sum(v.numel() for v in pre.values())
    for name, i, vh, vo, rms in fl[:20]:
        print("  sign flip: %s[%d] hip %+.3e fp64 oracle %+.3e (tensor rms %.3e)" % (name, i, vh, vo, rms))
    print("headline shape: %d pre-activations, %d flips (cap %d)" % (total, len(fl), ku.max_flips(total)))
    assert len(fl) <= ku.max_flips(total), (len(fl), total)
    for name, i, vh, vo, rms in fl:
        assert abs(vh) <= 1e-4 * rms and abs(vo) <= 1e-4 * rms, (name, i, vh, vo, rms)
    dx_ref = oracle_r2p1d(g, force=ku.sign_masks(pre))[1] if fl else dx_own
    e_pat, e_own = rel_max(xa.grad.cpu().numpy(), dx_ref.numpy()), rel_max(xa.grad.cpu().numpy(), dx_own.numpy())
    print("headline shape: max|dx - ref| / max|ref|: on the HIP pattern %.3e, on the oracle's own pattern %.3e" % (e_pat, e_own))
    assert e_pat <= 1e-3, e_pat


# ================================================================================================================ layer Grad-CAM
def test_layer_gradcam_conv3_matches_reference_recording(golden_dir):
    from src.visualization.visualize_cam import GradCAM_R2Plus1D
    g = load(golden_dir, "r2p1d_a")
    m, x = model_of(g)
    B, T, H, W = (int(v) for v in g["shape"])
    cam = GradCAM_R2Plus1D(m, layer="conv3")
    with arithmetic(True):
        maps, logits = cam.compute(x, 0)
        torch.cuda.synchronize()
    Cc, (Tq, h, w) = g["grad/conv3"].shape[1], g["grad/conv3"].shape[2:]
    dz = ku._to_ncthw(cam.dz, Cc, (B, Tq, h, w)).cpu().numpy()
    act = ku._to_ncthw(cam.act, Cc, (B, Tq, h, w)).cpu().numpy()
    print("conv3: dz %.3e act %.3e weights %.3e cam_raw %.3e map %.3e" % (
        rel_max(dz, g["grad/conv3"]), rel_max(act, g["act/conv3"]), rel_max(cam.weights.cpu().numpy(), g["alpha"]),
        rel_max(cam.cam_raw.cpu().numpy(), g["cam_raw"]), float(np.max(np.abs(maps.cpu().numpy() - g["map"])))))
    assert rel_max(dz, g["grad/conv3"]) <= 1e-3
    assert rel_max(cam.cam_raw.cpu().numpy(), g["cam_raw"]) <= 1e-3
    assert maps.shape == (B, H, W) and float(np.max(np.abs(maps.cpu().numpy() - g["map"]))) <= 1e-3
    img, heat, res, fig = GradCAM_R2Plus1D(m, layer="conv3")(x[:1].contiguous())
    assert img.shape == (H, W, 3) and heat.shape == (H, W, 3) and heat.dtype == np.uint8 and res.dtype == np.uint8
    if fig is not None:
        import matplotlib.pyplot as plt
        plt.close(fig)


def test_conv5_general_path_equals_special_case_and_default_is_unchanged(golden_dir):
    from src import _native as N
    from src.visualization import _xai
    from src.visualization.visualize_cam import GradCAM_R2Plus1D
    g = load(golden_dir, "r2p1d_a")
    m, x = model_of(g)
    B, T, H, W = (int(v) for v in g["shape"])
    cam = GradCAM_R2Plus1D(m)
    maps, logits = cam.compute(x, 0)
    raw = cam.cam_raw.clone()
    # the parent commit's code path, called as before: head gradient + md_gradcam on the last materialised tensor
    with torch.no_grad():
        feat = m.res2plus1d(x)
        h = m.linear
        dfeat = _xai.head_eval_dfeat(feat, h[0], h[1], h[3], float(h[2].alpha), 0)
        plan = m.res2plus1d._plan(B, T, H, W)
        z, Cc = plan.z_tensor(plan.eval_workspace(DEV), N.lib().md_plan_num_z(plan._h) - 1)
        last = plan.descs[-1]
        raw_old, maps_old = _xai.gradcam(z, Cc, last.To, last.Ho, last.Wo, dfeat, H, W)
    assert torch.equal(maps, maps_old) and torch.equal(raw, raw_old)
    gen = GradCAM_R2Plus1D(m, layer="conv5"); gen.general = True
    maps_g, _ = gen.compute(x, 0)
    torch.cuda.synchronize()
    print("conv5 general vs special: map %.3e" % float((maps_g - maps).abs().max()))
    assert float((maps_g - maps).abs().max()) <= 1e-5


# ================================================================================================================ SlowFast
@pytest.mark.parametrize("exact", [True, False], ids=["exact_fp32", "split"])
def test_slowfast_eval_input_gradient_matches_reference_recording(golden_dir, exact):
    from src.visualization.visualize_saliency import InputGradient
    g = load(golden_dir, "slowfast")
    m, sd, layers, x = slowfast_state(g)
    m.load_state_dict(sd, strict=True)
    m.to(DEV).eval()
    with arithmetic(exact):
        xa = x.to(DEV).requires_grad_(True)
        logits = m(xa)
        logits[:, 0].sum().backward()
        grad, maps, lg = InputGradient(m).compute(x.to(DEV), target=0)
        torch.cuda.synchronize()
    e = rel_max(xa.grad.cpu().numpy(), g["dx"])
    print("slowfast %s: logits %.3e dx %.3e (InputGradient %.3e)" % ("exact" if exact else "split",
          rel_max(logits.detach().cpu().numpy(), g["logits"]), e, rel_max(grad.cpu().numpy(), g["dx"])))
    assert rel_max(logits.detach().cpu().numpy(), g["logits"]) <= 1e-3
    assert e <= 1e-3 and rel_max(grad.cpu().numpy(), g["dx"]) <= 1e-3
    # (BatchNorm units and the head give no parameter gradients in eval mode; the plain lateral convolutions still do)
    assert all(p.grad is None for k, p in m.named_parameters() if ".bn" in k)
    assert maps.shape == (1,) + tuple(x.shape[2:]) and float(maps.min()) == 0.0 and float(maps.max()) == 1.0


@pytest.mark.parametrize("exact", [True, False], ids=["exact_fp32", "split"])
def test_gradcam_slowfast_matches_reference_recording(golden_dir, exact):
    from src.visualization.visualize_cam import GradCAM_SlowFast
    g = load(golden_dir, "slowfast")
    m, sd, layers, x = slowfast_state(g)
    m.load_state_dict(sd, strict=True)
    m.to(DEV).eval()
    cam = GradCAM_SlowFast(m)
    S = int(g["shape"][2])
    with arithmetic(exact):
        ms, mf, logits = cam.compute(x.to(DEV), 0)
        torch.cuda.synchronize()
    assert rel_max(logits.cpu().numpy(), g["logits"]) <= 1e-3
    assert rel_max(cam.input_grad.cpu().numpy(), g["dx"]) <= 1e-3
    for name, mp in (("slow", ms), ("fast", mf)):
        ref_a, ref_g = g["act/" + name], g["grad/" + name]
        Cc = ref_a.shape[1]
        act = cam.act[name][..., :Cc].permute(0, 4, 1, 2, 3).cpu().numpy()
        grad = cam.grad[name][..., :Cc].permute(0, 4, 1, 2, 3).cpu().numpy()
        emap = float(np.max(np.abs(mp.cpu().numpy() - recorded_map(g["map/" + name]))))
        print("slowfast %s %s: act %.3e grad %.3e cam_raw %.3e map %.3e" % ("exact" if exact else "split", name, rel_max(act, ref_a),
              rel_max(grad, ref_g), rel_max(cam.cam_raw[name].cpu().numpy(), g["cam_raw/" + name]), emap))
        assert act.shape == ref_a.shape and rel_max(act, ref_a) <= 1e-3
        assert rel_max(grad, ref_g) <= 1e-3
        assert mp.shape == (1, S, S) and emap <= 1e-3
    img, hs, hf, fig = cam(x.to(DEV))
    assert img.shape == (S, S, 3) and hs.shape == (S, S, 3) and hf.shape == (S, S, 3) and hs.dtype == np.uint8
    if fig is not None:
        import matplotlib.pyplot as plt
        plt.close(fig)


# ================================================================================================================ SmoothGrad
def test_smoothgrad_equals_mean_of_single_calls(golden_dir):
    from src.visualization.visualize_saliency import InputGradient
    g = load(golden_dir, "r2p1d_a")
    m, x = model_of(g)
    sal = InputGradient(m)
    gen = torch.Generator(device=DEV).manual_seed(77)
    grad, maps, logits = sal.compute(x, target=0, smooth=4, sigma=0.1, generator=gen)
    gen = torch.Generator(device=DEV).manual_seed(77)
    copies = InputGradient.noisy_copies(x, 4, 0.1, gen)
    span = float(x[0].max() - x[0].min())
    assert abs(float((copies[0][0] - x[0]).std()) / (0.1 * span) - 1.0) < 0.05          # noise of sigma x the clip's value range
    mean = torch.zeros_like(grad, dtype=torch.float64)
    for j in range(4):
        mean += sal.compute(copies[j], target=0)[0].double()
    mean /= 4
    torch.cuda.synchronize()
    e = float((grad.double() - mean).abs().max() / mean.abs().max())
    print("SmoothGrad n=4 vs mean of single calls: %.3e" % e)
    assert e <= 1e-6
    assert float(np.max(np.abs(maps.cpu().numpy() - saliency_map_ref(grad.cpu().numpy())))) <= 1e-6
    assert torch.equal(logits, sal.compute(x, target=0)[2])


# ================================================================================================================ nothing else moved
def test_training_step_after_eval_backward_is_bit_identical():
    from src.loss import FocalLoss
    ls, (B, T, H, W), seed = [1, 2, 2, 1], (2, 8, 64, 48), 1301
    x = clip(B, T, H, W, seed).to(DEV)
    y = torch.tensor([0, 1], device=DEV)

    def train_grads(with_eval_backward):
        m = r2p1d(ls, T, H, W, seed)
        if with_eval_backward:
            xa = x.clone().requires_grad_(True)
            m(xa)[:, 0].sum().backward()
            assert xa.grad is not None
        m.train()
        FocalLoss(weight=torch.ones(2), gamma=2.0)(m(x), y).backward()
        torch.cuda.synchronize()
        return {k: p.grad.clone() for k, p in m.named_parameters()}, {k: v.clone() for k, v in m.state_dict().items() if "running" in k}

    ga, sa = train_grads(False)
    gb, sb = train_grads(True)
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


def test_input_grad_refuses_a_training_workspace():
    m = r2p1d([1, 1, 1, 1], 8, 48, 40, 1201)
    net = m.res2plus1d
    x = clip(1, 8, 48, 40, 5).to(DEV)
    plan = net._plan(1, 8, 48, 40)
    units = net.unit_modules()
    ws = plan.new_workspace(DEV)
    args = ([u.conv.weight for u in units], [u.bn.weight for u in units], [u.bn.bias for u in units],
            [u.bn.running_mean.clone() for u in units], [u.bn.running_var.clone() for u in units])
    plan.forward(x, ws, *args, True)
    with pytest.raises(RuntimeError, match="unsupported"):
        plan.input_grad(torch.ones(1, 128, device=DEV), ws, args[0])
    plan.forward(x, ws, *args, False)
    dx, _ = plan.input_grad(torch.ones(1, 128, device=DEV), ws, args[0])
    torch.cuda.synchronize()
    assert torch.isfinite(dx).all()
