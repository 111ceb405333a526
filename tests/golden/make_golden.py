#!/usr/bin/env python3
"""Generate the golden fixtures in this directory from the REFERENCE implementation.

Run in the build container only (needs /root/reference; never on the GPU box):

    python tests/golden/make_golden.py

The reference is imported unmodified; modules it needs that are absent here and play no
part in the arithmetic (pytorch_model_summary, seaborn, tensorboard) are replaced by empty
stand-ins in ``sys.modules``.  Inputs and weights come from the NumPy recipes in
``oracle/r2plus1d.py`` (``synth_state``/``synth_clip``/``synth_labels``) and are loaded into
the reference modules with ``load_state_dict`` -- so a fixture stores only the recipe's seed,
the reference's OUTPUTS, and sub-sampled gradients (data, no reference source).
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


class _NoWriter:
    def __init__(self, *a, **k):
        pass

    def __getattr__(self, name):
        return lambda *a, **k: None


_stub("torch.utils.tensorboard", SummaryWriter=_NoWriter)

sys.path.insert(0, REF)     # the reference's own `src` package
sys.path.insert(1, ROOT)    # oracle/ (weight + input recipes only)

from oracle import r2plus1d as orc          # noqa: E402
from src.models.R2Plus1D import R2Plus1DClassifier   # noqa: E402  (reference)
from src.loss import FocalLoss, LDAMLoss, CELoss      # noqa: E402  (reference)

torch.set_num_threads(8)


def subsample(t: torch.Tensor, n: int = 48) -> np.ndarray:
    f = t.detach().reshape(-1)
    stride = max(1, f.numel() // n)
    return f[::stride][:n].numpy().copy()


def load_ref_model(layer_sizes, T, S, alpha, seed):
    model = R2Plus1DClassifier(input_size=(3, T, S, S), num_classes=2, layer_sizes=layer_sizes, alpha=alpha)
    params, bufs = orc.synth_state(layer_sizes, seed, alpha)
    sd = {}
    sd.update(params)
    sd.update(bufs)
    missing, unexpected = model.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    return model


def model_fixture(tag, layer_sizes, B, T, S, alpha, seed, gamma=2.0, weight=(1.0, 1.0)):
    model = load_ref_model(layer_sizes, T, S, alpha, seed)
    model.train()
    x = orc.synth_clip(B, T, S, seed)
    y = orc.synth_labels(B, seed)
    loss_fn = FocalLoss(weight=torch.tensor(weight, dtype=torch.float32), gamma=gamma)
    feats = {}
    h = model.res2plus1d.conv1.register_forward_hook(lambda m, i, o: feats.__setitem__("stem", o.detach()))
    h2 = model.res2plus1d.register_forward_hook(lambda m, i, o: feats.__setitem__("trunk", o.detach()))
    logits = model(x)
    h.remove(); h2.remove()
    loss = loss_fn(logits, y)
    loss.backward()
    out = {
        "layer_sizes": np.array(layer_sizes), "B": B, "T": T, "S": S, "alpha": alpha, "seed": seed,
        "gamma": gamma, "weight": np.array(weight, dtype=np.float32),
        "logits": logits.detach().numpy(), "loss": loss.detach().numpy(),
        "trunk": feats["trunk"].numpy(),
        "stem_sub": subsample(feats["stem"], 256),
        "stem_mean": feats["stem"].mean().numpy(), "stem_std": feats["stem"].std().numpy(),
    }
    names = []
    for k, p in model.named_parameters():
        names.append(k)
        out["gsub/" + k] = subsample(p.grad)
        out["gnorm/" + k] = np.float32(p.grad.norm().item())
    out["param_names"] = np.array(names)
    # the reference's own fp32 rounding noise on these gradients: same code, fp64
    m64 = load_ref_model(layer_sizes, T, S, alpha, seed).double()
    m64.train()
    l64 = FocalLoss(weight=torch.tensor(weight, dtype=torch.float64), gamma=gamma)(m64(x.double()), y)
    l64.backward()
    noise = 0.0
    gmax = max(float(p.grad.norm()) for p in m64.parameters())
    for (k, p), (_, q) in zip(model.named_parameters(), m64.named_parameters()):
        if k == "linear.0.bias":
            continue
        sc = max(float(q.grad.abs().max()), 1e-5 * gmax)
        noise = max(noise, float((p.grad.double() - q.grad).abs().max()) / sc)
    out["ref_noise"] = np.float64(noise)
    print(f"  {tag}: reference fp32-vs-fp64 gradient deviation {noise:.2e}")
    sd = model.state_dict()
    for k in ("res2plus1d.conv1.spatio_conv.bn.running_mean", "res2plus1d.conv1.spatio_conv.bn.running_var",
              "res2plus1d.conv5.block1.conv2.temporal_conv.bn.running_var", "linear.1.running_mean",
              "linear.1.running_var"):
        out["buf/" + k] = sd[k].numpy().copy()
    out["nbt"] = sd["linear.1.num_batches_tracked"].numpy()
    np.savez_compressed(os.path.join(HERE, tag + ".npz"), **out)
    print(tag, "logits", logits.detach().numpy().ravel(), "loss", float(loss))


def loss_fixture():
    rng = np.random.default_rng(11)
    out = {}
    for B in (1, 8, 33):
        x = torch.from_numpy((rng.standard_normal((B, 2)) * 2.5).astype("float32"))
        y = torch.from_numpy(rng.integers(0, 2, size=B).astype("int64"))
        w = torch.tensor([1.7, 0.3])
        out[f"x{B}"] = x.numpy(); out[f"y{B}"] = y.numpy(); out["w"] = w.numpy()
        for name, fn in (
            ("focal_g2", FocalLoss(weight=w, gamma=2.0)),
            ("focal_g0p5", FocalLoss(weight=w, gamma=0.5)),
            ("ldam_s30", LDAMLoss([100, 2000], max_m=0.5, weight=w, s=30)),
            ("ldam_s1_now", LDAMLoss([100, 2000], max_m=0.5, weight=None, s=1)),
            ("ce", CELoss(weight=w)),
        ):
            xx = x.clone().requires_grad_(True)
            L = fn(xx, y)
            L.backward()
            out[f"{name}/L{B}"] = L.detach().numpy()
            out[f"{name}/g{B}"] = xx.grad.numpy()
    out["m_list"] = LDAMLoss([100, 2000], max_m=0.5).m_list.numpy()
    # Gradient blending (reference: src/GradientBlending.py:45-50)
    from src.GradientBlending import GradientBlending
    B = 8
    xs = [torch.from_numpy(rng.standard_normal((B, 2)).astype("float32")).requires_grad_(True) for _ in range(3)]
    y = torch.from_numpy(rng.integers(0, 2, size=B).astype("int64"))
    w = torch.tensor([1.0, 1.0])
    gb = GradientBlending(FocalLoss(w, 2.0), FocalLoss(w, 2.0), FocalLoss(w, 2.0), 0.1, 0.4, 0.5)
    L = gb(xs[0], xs[1], xs[2], y)
    L.backward()
    out["gb/y"] = y.numpy()
    for i, n in enumerate(("multi", "vis", "ts")):
        out[f"gb/x_{n}"] = xs[i].detach().numpy(); out[f"gb/g_{n}"] = xs[i].grad.numpy()
    out["gb/L"] = L.detach().numpy()
    np.savez_compressed(os.path.join(HERE, "losses.npz"), **out)
    print("losses ok")


def drw_fixture():
    # DRW schedule: the weight table is computed by a closure inside the reference's train_DRW
    # (src/train.py:318-329), so it cannot be called on its own.  Run train_DRW for real on a 1-batch
    # synthetic loader with a loss object that records every update_weight() call.
    from src.train import train_DRW
    torch.autograd.set_detect_anomaly(False)
    rec = {}

    class RecLoss(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.model_type = "Focal"
            self.cur = None

        def update_weight(self, w):
            self.cur = w.detach().cpu().numpy().copy()
            self.log.append(self.cur)

        def forward(self, out, tgt):
            return torch.nn.functional.cross_entropy(out, tgt, reduction="sum")

    lin = torch.nn.Linear(4, 2)
    data = [(torch.randn(4, 4), torch.tensor([0, 1, 1, 0]))]
    for num_epoch in (8, 50, 128):
        lf = RecLoss(); lf.log = []
        opt = torch.optim.SGD(lin.parameters(), lr=0.0)
        train_DRW(data, data, lin, opt, lf, "cpu", num_epoch, verbose=None,
                  save_best_dir="/tmp/_g_best.pt", save_last_dir="/tmp/_g_last.pt", exp_dir="/tmp/_g_exp",
                  max_norm_grad=1.0, betas=[0, 0.25, 0.75, 0.9], cls_num_list=[100, 2000])
        rec[f"w{num_epoch}"] = np.stack(lf.log)
    np.savez_compressed(os.path.join(HERE, "drw.npz"), **rec)
    print("drw ok", {k: v.shape for k, v in rec.items()})


def step_fixture():
    """train_per_epoch (reference src/train.py:17-93) on 3 fixed batches of a tiny R2Plus1D."""
    from src.train import train_per_epoch
    torch.autograd.set_detect_anomaly(False)
    layer_sizes, B, T, S, alpha, seed = [1, 1, 1, 1], 4, 4, 32, 0.01, 5
    model = load_ref_model(layer_sizes, T, S, alpha, seed)
    batches = [(orc.synth_clip(B, T, S, seed + i), orc.synth_labels(B, seed + i, 0.4)) for i in range(3)]
    opt = torch.optim.AdamW(model.parameters(), lr=2e-4)
    loss_fn = FocalLoss(weight=torch.tensor([1.0, 1.0]), gamma=2.0)
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    preds = []
    hook = model.register_forward_hook(lambda m, i, o: preds.append(torch.softmax(o, 1).max(1)[1].numpy().copy()))
    tl, ta, tf = train_per_epoch(batches, model, opt, None, loss_fn, "cpu", 1.0, "single")
    hook.remove()
    out = {"layer_sizes": np.array(layer_sizes), "B": B, "T": T, "S": S, "alpha": alpha, "seed": seed,
           "train_loss": np.float64(tl), "train_acc": np.float64(ta), "train_f1": np.float64(tf),
           "preds": np.stack(preds)}
    for k, p in model.named_parameters():
        out["dsub/" + k] = subsample(p.detach() - before[k])
    np.savez_compressed(os.path.join(HERE, "step_tiny.npz"), **out)
    print("step", tl, ta, tf, np.stack(preds))


def elementwise_fixture():
    """SwishEfficient (resnet.py:70-81) forward/backward and NoiseLayer (NoiseLayer.py:5-16) outputs of the reference."""
    from src.models.resnet import SwishEfficient
    from src.models.NoiseLayer import NoiseLayer
    rng = np.random.default_rng(2024)
    x = np.concatenate([rng.standard_normal(4093).astype(np.float32) * 3.0,
                        np.array([0.0, -0.0, 1e-8, -1e-8, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0], dtype=np.float32)])
    dy = rng.standard_normal(x.shape[0]).astype(np.float32)
    xt = torch.from_numpy(x).requires_grad_(True)
    y = SwishEfficient.apply(xt)
    y.backward(torch.from_numpy(dy))
    out = {"swish_x": x, "swish_dy": dy, "swish_y": y.detach().numpy(), "swish_dx": xt.grad.numpy()}
    xn = rng.standard_normal((6, 21, 14)).astype(np.float32)
    layer = NoiseLayer(mean=0.05, std=1e-2)
    layer.train()
    torch.manual_seed(777)
    out["noise_x"] = xn
    out["noise_seed"] = np.int64(777); out["noise_mean"] = np.float32(0.05); out["noise_std"] = np.float32(1e-2)
    out["noise_train"] = layer(torch.from_numpy(xn)).numpy()
    layer.eval()
    out["noise_eval"] = layer(torch.from_numpy(xn)).numpy()
    np.savez_compressed(os.path.join(HERE, "elementwise.npz"), **out)
    print("elementwise", float(np.abs(out["swish_y"]).max()), float(np.abs(out["noise_train"] - xn).mean()))


def bottleneck_fixture(tag, in_planes, planes, stride, head_conv, index, with_ds, shape, seed):
    """Bottleneck3D (resnet.py:121-200) of the reference: state dict (its own seeded init, BN affine randomised so that the
    scale/shift paths are exercised), input, output, input gradient, parameter gradients, running statistics after the step."""
    from src.models.resnet import Bottleneck3D
    import torch.nn as nn
    torch.manual_seed(seed)
    ds = None
    if with_ds:
        ds = nn.Sequential(nn.Conv3d(in_planes, planes * 4, kernel_size=1, stride=(1, stride, stride), bias=False),
                           nn.BatchNorm3d(planes * 4))
    m = Bottleneck3D(in_planes, planes, stride, ds, head_conv=head_conv, index=index)
    with torch.no_grad():
        for k, v in m.named_parameters():
            if ".weight" in k and v.dim() == 1:
                v.uniform_(0.5, 1.5)
            elif k.endswith(".bias") and ("bn" in k or "downsample.1" in k):
                v.normal_(0.0, 0.3)
    sd0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m.train()
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(*shape, generator=g).requires_grad_(True)
    out = m(x)
    dout = torch.randn(out.shape, generator=g)
    out.backward(dout)
    rec = {"in_planes": in_planes, "planes": planes, "stride": stride, "head_conv": head_conv, "index": index,
           "with_ds": int(with_ds), "x": x.detach().numpy(), "dout": dout.numpy(), "out": out.detach().numpy(),
           "dx": x.grad.numpy()}
    for k, v in sd0.items():
        rec["sd/" + k] = v.numpy()
    for k, p in m.named_parameters():
        rec["grad/" + k] = p.grad.numpy()
    for k, v in m.state_dict().items():
        if "running" in k:
            rec["after/" + k] = v.numpy()
    np.savez_compressed(os.path.join(HERE, tag + ".npz"), **rec)
    print(tag, tuple(out.shape), float(out.abs().max()))


def slowfast_fixture():
    """SlowFast (slowfast.py:165-196) of the reference at a tiny configuration.  Weights and the input come from the NumPy
    recipes in oracle/slowfast.py (loaded with load_state_dict), so the fixture stores seeds plus the reference's logits,
    sub-sampled gradients, gradient norms and the running statistics after one training-mode step."""
    from src.models.slowfast import SlowFast
    from oracle import slowfast as osf
    layers, T, S, B, seed = [1, 1, 1, 1], 8, 64, 3, 41
    m = SlowFast(input_shape=(3, T, S, S), layers=layers, alpha=4, tau_fast=1, num_classes=2, alpha_elu=1.0)
    sd0 = osf.synth_state({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed)
    m.load_state_dict(sd0, strict=True)
    m.train()
    x = osf.synth_clip(B, T, S, seed + 1)
    logits = m(x)
    dlog = torch.from_numpy(np.random.default_rng(seed + 2).standard_normal(tuple(logits.shape)).astype(np.float32))
    logits.backward(dlog)
    rec = {"layers": np.array(layers), "T": T, "S": S, "B": B, "seed": seed, "dlogits": dlog.numpy(),
           "logits": logits.detach().numpy()}
    for k, p in m.named_parameters():
        rec["gsub/" + k] = subsample(p.grad)
        rec["gnorm/" + k] = np.float64(p.grad.double().norm())
    for k, v in m.state_dict().items():
        if "running" in k:
            rec["after/" + k] = v.numpy()
    np.savez_compressed(os.path.join(HERE, "slowfast_tiny.npz"), **rec)
    print("slowfast", logits.detach().numpy())


def gb_loops_fixture():
    """GB_estimate (GradientBlending.py:52-114) and train_GB_dynamic (:310-446) of the reference on the tiny two-stream model
    and loaders of oracle/fake_multimodal.py (CPU, SGD, summed cross entropy): the estimated weights, the loss histories and
    the final blending weights."""
    import tempfile
    from src.GradientBlending import GB_estimate, GradientBlending, train_GB_dynamic
    from oracle.fake_multimodal import FakeMultiModalGB, loaders
    ce = lambda: torch.nn.CrossEntropyLoss(reduction="sum")
    with tempfile.TemporaryDirectory() as d:
        tr, va = loaders(11)
        model = FakeMultiModalGB()
        last = os.path.join(d, "last.pt"); best = os.path.join(d, "best.pt")
        torch.save(model.state_dict(), last)
        opt = torch.optim.SGD(model.parameters(), lr=0.05)
        w = GB_estimate(2, tr, va, last, model, opt, None, ce(), "cpu", None)
        rec = {"est/" + k: np.float64(v) for k, v in w.items()}
        model = FakeMultiModalGB()
        opt = torch.optim.SGD(model.parameters(), lr=0.05)
        loss_gb = GradientBlending(ce(), ce(), ce(), 0.2, 0.3, 0.5, 1.0)
        hist = train_GB_dynamic(tr, va, model, opt, None, loss_gb, ce(), "cpu", num_epoch=4, epoch_per_GB_estimate=2,
                                num_epoch_GB_estimate=2, verbose=None, save_best_dir=best, save_last_dir=last,
                                exp_dir=os.path.join(d, "exp"), max_norm_grad=1.0, criteria="loss")
        for name, h in zip(("train_loss", "train_acc", "train_f1", "valid_loss", "valid_acc", "valid_f1"), hist):
            rec["dyn/" + name] = np.array(h, dtype=np.float64)
        rec["dyn/weights"] = np.array([loss_gb.vis_weight, loss_gb.ts_weight, loss_gb.vis_ts_weight], dtype=np.float64)
        # train_GB (:165-308, fixed weights, criteria "acc") and evaluate_GB (:116-163: macro-F1 of the three heads)
        from src.GradientBlending import train_GB, evaluate_GB
        model = FakeMultiModalGB(); model.update_use_stream("multi-GB")
        opt = torch.optim.SGD(model.parameters(), lr=0.05)
        loss_gb = GradientBlending(ce(), ce(), ce(), 0.2, 0.3, 0.5, 1.0)
        hist = train_GB(tr, va, model, opt, None, loss_gb, "cpu", num_epoch=3, verbose=None, save_best_dir=best, save_last_dir=last,
                        exp_dir=os.path.join(d, "exp2"), max_norm_grad=1.0, criteria="acc")
        for name, h in zip(("train_loss", "train_acc", "train_f1", "valid_loss", "valid_acc", "valid_f1"), hist):
            rec["fix/" + name] = np.array(h, dtype=np.float64)
        rec["fix/evalgb_train"] = np.array(evaluate_GB(tr, model, opt, "cpu", 0.5), dtype=np.float64)
        rec["fix/evalgb_valid"] = np.array(evaluate_GB(va, model, opt, "cpu", 0.5), dtype=np.float64)
        best_sd = torch.load(best, weights_only=True)
        rec["fix/best_head_bias"] = best_sd["head.bias"].double().numpy()
    np.savez_compressed(os.path.join(HERE, "gb_loops.npz"), **rec)
    print("gb loops", w, rec["dyn/weights"])


def cnnlstm_fixture():
    """CnnLSTM (CnnLSTM.py:10-109) of the reference (its own seeded init; noise std set to 0 so that the run is deterministic
    without sharing the CPU generator state): state dict, input, logits, input gradient, parameter gradients, running stats."""
    from src.models.CnnLSTM import CnnLSTM
    torch.manual_seed(51)
    m = CnnLSTM(seq_len=21, n_features=12, conv_dim=32, conv_kernel=3, conv_stride=1, conv_padding=1, lstm_dim=32, n_layers=2,
                bidirectional=True, n_classes=2)
    m.noise.std = 0.0
    with torch.no_grad():
        m.conv[2].weight.uniform_(0.5, 1.5); m.conv[2].bias.normal_(0, 0.3)
        m.classifier[1].weight.uniform_(0.5, 1.5); m.classifier[1].bias.normal_(0, 0.3)
    sd0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m.train()
    g = torch.Generator().manual_seed(52)
    x = torch.randn(6, 21, 12, generator=g).requires_grad_(True)
    out = m(x)
    dout = torch.randn(out.shape, generator=g)
    out.backward(dout)
    rec = {"x": x.detach().numpy(), "dout": dout.numpy(), "out": out.detach().numpy(), "dx": x.grad.numpy()}
    for k, v in sd0.items():
        rec["sd/" + k] = v.numpy()
    for k, p in m.named_parameters():
        rec["grad/" + k] = p.grad.numpy()
    for k, v in m.state_dict().items():
        if "running" in k:
            rec["after/" + k] = v.numpy()
    np.savez_compressed(os.path.join(HERE, "cnnlstm.npz"), **rec)
    print("cnnlstm", out.detach().numpy()[:2], float(m.w_s1.weight.grad.abs().max()))


def mlstm_fcn_fixture():
    """MLSTM_FCN (MLSTM_FCN.py:84-169) of the reference (its own seeded init; noise std and LSTM dropout 0 for determinism):
    state dict, input, logits, input gradient, parameter gradients, running statistics."""
    from src.models.MLSTM_FCN import MLSTM_FCN
    torch.manual_seed(61)
    m = MLSTM_FCN(n_features=14, fcn_dim=32, kernel_size=3, stride=1, seq_len=21, lstm_dim=24, lstm_n_layers=2,
                  lstm_bidirectional=True, lstm_dropout=0.0, reduction=16, alpha=0.01, n_classes=2)
    m.noise.std = 0.0
    with torch.no_grad():
        for k, v in m.named_parameters():
            if ".bn." in k or k.startswith("classifier.1."):
                (v.uniform_(0.5, 1.5) if k.endswith("weight") else v.normal_(0, 0.3))
    sd0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m.train()
    g = torch.Generator().manual_seed(62)
    x = torch.randn(8, 21, 14, generator=g).requires_grad_(True)
    out = m(x)
    dout = torch.randn(out.shape, generator=g)
    out.backward(dout)
    rec = {"x": x.detach().numpy(), "dout": dout.numpy(), "out": out.detach().numpy(), "dx": x.grad.numpy()}
    for k, v in sd0.items():
        rec["sd/" + k] = v.numpy()
    for k, p in m.named_parameters():
        rec["grad/" + k] = p.grad.numpy()
    for k, v in m.state_dict().items():
        if "running" in k:
            rec["after/" + k] = v.numpy()
    np.savez_compressed(os.path.join(HERE, "mlstm_fcn.npz"), **rec)
    print("mlstm_fcn", out.detach().numpy()[:2])


def transformer0d_fixture():
    """Transformer (transformer.py:112-154) of the reference (its own seeded init; noise std and dropout 0 for determinism): state
    dict, input, logits, input gradient, parameter gradients, running statistics."""
    from src.models.transformer import Transformer
    torch.manual_seed(71)
    m = Transformer(n_features=18, kernel_size=5, feature_dims=64, max_len=21, n_layers=2, n_heads=4, dim_feedforward=96, dropout=0.0,
                    cls_dims=32, n_classes=2)
    m.encoder.noise.std = 0.0
    with torch.no_grad():
        for k, v in m.named_parameters():
            if "norm" in k or "filter.2" in k or k.endswith("connector.1.weight") or k.endswith("connector.1.bias") or k.startswith("classifier.1"):
                (v.uniform_(0.5, 1.5) if k.endswith("weight") else v.normal_(0, 0.3))
    sd0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m.train()
    g = torch.Generator().manual_seed(72)
    x = torch.randn(8, 21, 18, generator=g).requires_grad_(True)
    out = m(x)
    dout = torch.randn(out.shape, generator=g)
    out.backward(dout)
    rec = {"x": x.detach().numpy(), "dout": dout.numpy(), "out": out.detach().numpy(), "dx": x.grad.numpy()}
    for k, v in sd0.items():
        rec["sd/" + k] = v.numpy()
    for k, p in m.named_parameters():
        rec["grad/" + k] = p.grad.numpy()
    for k, v in m.state_dict().items():
        if "running" in k:
            rec["after/" + k] = v.numpy()
    np.savez_compressed(os.path.join(HERE, "transformer0d.npz"), **rec)
    print("transformer0d", out.detach().numpy()[:2])


def vivit_fixture():
    """ViViT (pool cls, with mlp) and ViViTEncoder (pool mean) of the reference (ViViT.py:115-299; its own seeded init with the
    LayerNorm parameters moved off 1/0; dropout 0): state dict, clip, output, input gradient, parameter gradients."""
    from src.models.ViViT import ViViT, ViViTEncoder
    rec = {}
    for tag, cls, kw, seed in (("cls", ViViT, dict(n_classes=2, pool="cls", alpha=0.7), 81), ("enc", ViViTEncoder, dict(pool="mean"), 83)):
        torch.manual_seed(seed)
        m = cls(image_size=32, patch_size=8, n_frames=5, dim=32, depth=2, n_heads=2, in_channels=3, d_head=16, dropout=0.0,
                embedd_dropout=0.0, scale_dim=2, **kw)
        with torch.no_grad():
            for k, v in m.named_parameters():
                if "norm" in k or k.startswith("mlp.1"):
                    (v.uniform_(0.5, 1.5) if k.endswith("weight") else v.normal_(0, 0.3))
        m.train()
        g = torch.Generator().manual_seed(seed + 1)
        x = torch.randn(3, 5, 3, 32, 32, generator=g).requires_grad_(True)           # (b, t, c, H, W)
        out = m(x)
        dout = torch.randn(out.shape, generator=g)
        out.backward(dout)
        rec.update({tag + "/x": x.detach().numpy(), tag + "/dout": dout.numpy(), tag + "/out": out.detach().numpy(),
                    tag + "/dx": x.grad.numpy()})
        for k, v in m.state_dict().items():
            rec[tag + "/sd/" + k] = v.detach().numpy()
        for k, p in m.named_parameters():
            rec[tag + "/grad/" + k] = p.grad.numpy()
        print("vivit", tag, out.detach().numpy().ravel()[:4])
    for tag in ("cls", "enc"):          # one file per case, so that each stays under 1 MiB
        np.savez_compressed(os.path.join(HERE, "vivit_%s.npz" % tag), **{k: v for k, v in rec.items() if k.split("/")[0] == tag})


def multimodal_fixture():
    """The four fusion wrappers of the reference (MultiModal.py:10-331) on tiny encoders (noise std 0, dropout 0; LayerNorm /
    BatchNorm parameters moved off 1/0): state dict, inputs, outputs, parameter gradients of sum_k <out_k, dout_k>, running
    statistics afterwards.  The *_GB classes need Transformer.feature_dims, which the reference never sets: the
    attribute is supplied on the imported class, nothing else is touched."""
    from src.models import MultiModal as MM
    from src.models.transformer import Transformer
    Transformer.feature_dims = property(lambda self: self.encoder.feature_dims)
    av = dict(image_size=32, patch_size=8, n_frames=5, dim=16, depth=1, n_heads=2, in_channels=3, d_head=8, dropout=0.0,
              embedd_dropout=0.0, scale_dim=2)
    a0 = dict(n_features=6, kernel_size=3, feature_dims=16, max_len=5, n_layers=1, n_heads=2, dim_feedforward=24, dropout=0.0)
    avg = dict(av, n_classes=2, pool="cls", alpha=1.0)
    a0g = dict(a0, cls_dims=12, n_classes=2)
    rec = {}
    for tag, cls, v, z, seed in (("mm", MM.MultiModalModel, dict(av, pool="mean"), a0, 91), ("gb", MM.MultiModalModel_GB, avg, a0g, 92),
                                 ("tfn", MM.TFN, dict(av, pool="mean"), a0, 93), ("tfngb", MM.TFN_GB, avg, a0g, 94)):
        torch.manual_seed(seed)
        m = cls(2, dict(v), dict(z))
        for mod in m.modules():
            if type(mod).__name__ == "NoiseLayer":
                mod.std = 0.0
        with torch.no_grad():
            for k, p in m.named_parameters():
                if p.dim() == 1 and (".norm" in k or "filter.2" in k or "connector.1" in k or "classifier.1" in k or "mlp.1" in k):
                    (p.uniform_(0.5, 1.5) if k.endswith("weight") else p.normal_(0, 0.3))
        sd0 = {k: t.detach().clone() for k, t in m.state_dict().items()}
        m.train()
        g = torch.Generator().manual_seed(seed + 100)
        x_vis = torch.randn(4, 3, 5, 32, 32, generator=g)                 # (B, C, T, H, W), as the loaders deliver it
        x_ts = torch.randn(4, 5, 6, generator=g)
        outs = m(x_vis, x_ts)
        outs = outs if isinstance(outs, tuple) else (outs,)
        douts = [torch.randn(o.shape, generator=g) for o in outs]
        sum((o * d).sum() for o, d in zip(outs, douts)).backward()
        rec[tag + "/x_vis"] = x_vis.numpy(); rec[tag + "/x_ts"] = x_ts.numpy()
        for i, (o, d) in enumerate(zip(outs, douts)):
            rec["%s/out%d" % (tag, i)] = o.detach().numpy(); rec["%s/dout%d" % (tag, i)] = d.numpy()
        for k, t in sd0.items():
            rec[tag + "/sd/" + k] = t.numpy()
        for k, p in m.named_parameters():
            rec[tag + "/grad/" + k] = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy()
        for k, t in m.state_dict().items():
            if "running" in k:
                rec[tag + "/after/" + k] = t.numpy()
        print("multimodal", tag, [o.detach().numpy().ravel()[:2] for o in outs])
    for tag in ("mm", "gb", "tfn", "tfngb"):          # one file per case, so that each stays under 1 MiB
        np.savez_compressed(os.path.join(HERE, "multimodal_%s.npz" % tag), **{k: v for k, v in rec.items() if k.split("/")[0] == tag})


def fusion_derived_fixture():
    """DERIVED fusion models for BASELINE configs 4 and 5: the reference's own R2Plus1DClassifier + Transformer, and
    SlowFast + MLSTM_FCN, combined by the recipe of its MultiModalModel_GB (MultiModal.py:65-77,96-97,131-149: forward hooks on
    the first Linear of each head capture the latents; connector Linear+ReLU; classifier Linear, LayerNorm, ReLU, Linear).
    Weights from the NumPy recipe oracle.fusion.fusion_state (seed stored, not megabytes), tiny shapes, noise std / dropout 0.
    Stored: inputs, the three logit sets, the blended loss (GradientBlending, :45-50) and sub-sampled gradients + norms."""
    import torch.nn as nn
    from src.models.slowfast import SlowFast
    from src.models.transformer import Transformer
    from src.models.MLSTM_FCN import MLSTM_FCN
    from src.GradientBlending import GradientBlending
    from oracle import fusion as ofu

    class DerivedGB(nn.Module):
        def __init__(self, vis, ts, vis_first_linear, ts_first_linear, dims):
            super().__init__()
            self.vis_model, self.ts_model = vis, ts
            self.connector = nn.Sequential(nn.Linear(dims, dims // 2), nn.ReLU())
            self.classifier = nn.Sequential(nn.Linear(dims // 2, dims // 2), nn.LayerNorm(dims // 2), nn.ReLU(), nn.Linear(dims // 2, 2))
            self.lat = {}
            vis_first_linear.register_forward_hook(lambda m, i, o: self.lat.__setitem__("vis", i))
            ts_first_linear.register_forward_hook(lambda m, i, o: self.lat.__setitem__("ts", i))

        def forward(self, x_vis, x_ts):
            out_vis = self.vis_model(x_vis)
            out_ts = self.ts_model(x_ts)
            x = torch.cat([self.lat["vis"][0], self.lat["ts"][0]], axis=1)
            return self.classifier(self.connector(x)), out_vis, out_ts

    rec = {}
    for tag, seed in (("cfg4", 101), ("cfg5", 111)):
        torch.manual_seed(seed)
        if tag == "cfg4":
            vis = R2Plus1DClassifier(input_size=(3, 5, 24, 24), num_classes=2, layer_sizes=[1, 1, 1, 1], alpha=0.01)
            ts = Transformer(n_features=6, kernel_size=3, feature_dims=16, max_len=5, n_layers=1, n_heads=2, dim_feedforward=24,
                             dropout=0.0, cls_dims=12, n_classes=2)
            m = DerivedGB(vis, ts, vis.linear[0], ts.classifier[0], 128 + 16)
            x_vis = torch.randn(4, 3, 5, 24, 24, generator=torch.Generator().manual_seed(seed + 1))
            x_ts = torch.randn(4, 5, 6, generator=torch.Generator().manual_seed(seed + 2))
            loss_fn = FocalLoss(torch.tensor([1.0, 1.0]), 2.0)
        else:
            vis = SlowFast(input_shape=(3, 8, 32, 32), layers=[1, 1, 1, 1], alpha=4, tau_fast=1, num_classes=2, alpha_elu=1.0)
            ts = MLSTM_FCN(n_features=6, fcn_dim=8, kernel_size=3, stride=1, seq_len=8, lstm_dim=8, lstm_n_layers=1,
                           lstm_bidirectional=True, lstm_dropout=0.0, reduction=4, alpha=0.01, n_classes=2)
            m = DerivedGB(vis, ts, vis.classifier.classifier[0], ts.classifier[0], vis.classifier.input_dim + ts.converter.out_features)
            x_vis = torch.randn(4, 3, 8, 32, 32, generator=torch.Generator().manual_seed(seed + 1))
            x_ts = torch.randn(4, 8, 6, generator=torch.Generator().manual_seed(seed + 2))
            loss_fn = LDAMLoss([100, 2000], max_m=0.5, weight=torch.tensor([1.0, 1.0]), s=1.0)
        for mod in m.modules():
            if type(mod).__name__ == "NoiseLayer":
                mod.std = 0.0
        m.load_state_dict(ofu.fusion_state({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed), strict=False)
        m.train()
        y = torch.tensor([0, 1, 1, 0])
        outs = m(x_vis, x_ts)
        gb = GradientBlending(loss_fn, loss_fn, loss_fn, 0.1, 0.4, 0.5)
        L = gb(outs[0], outs[1], outs[2], y)
        L.backward()
        rec.update({tag + "/seed": seed, tag + "/x_vis": x_vis.numpy(), tag + "/x_ts": x_ts.numpy(), tag + "/y": y.numpy(),
                    tag + "/loss": L.detach().numpy()})
        for i, o in enumerate(outs):
            rec["%s/out%d" % (tag, i)] = o.detach().numpy()
        for k, v in m.state_dict().items():
            rec[tag + "/shape/" + k] = np.array(tuple(v.shape), dtype=np.int64)
            if "running" in k:
                rec[tag + "/after/" + k] = v.numpy()
        for k, p in m.named_parameters():
            g = p.grad if p.grad is not None else torch.zeros_like(p)
            rec[tag + "/gsub/" + k] = subsample(g)
            rec[tag + "/gnorm/" + k] = np.float64(g.double().norm())
        print("fusion_derived", tag, float(L), [o.detach().numpy().ravel()[:2] for o in outs])
    np.savez_compressed(os.path.join(HERE, "fusion_derived.npz"), **rec)


if __name__ == "__main__":
    # Several seeds per configuration: LeakyReLU(0.01) makes the gradient discontinuous where a
    # pre-activation crosses zero, so two correct fp32 implementations can disagree by >1e-3 on a whole
    # gradient when ONE element (|x| < ~1e-6) lands on the other side of the kink.  Each fixture therefore
    # also records `ref_noise`: the largest deviation between the reference run in fp32 and the SAME
    # reference code run in fp64 (model.double()).  Seeds 3 and 11 show such a flip inside the reference.
    for seed in (1, 2, 3, 4):
        model_fixture(f"r2p1d_1111_s{seed}", [1, 1, 1, 1], B=4, T=5, S=24, alpha=0.01, seed=seed)
    model_fixture("r2p1d_1221_s11", [1, 2, 2, 1], B=4, T=6, S=24, alpha=1.0, seed=11, gamma=2.0, weight=(0.6, 1.4))
    model_fixture("r2p1d_1221_s12", [1, 2, 2, 1], B=5, T=7, S=24, alpha=0.2, seed=12, gamma=1.5, weight=(1.0, 1.0))
    model_fixture("r2p1d_1221_s13", [1, 2, 2, 1], B=4, T=4, S=32, alpha=0.01, seed=13, gamma=2.0, weight=(1.0, 1.0))
    loss_fixture()
    drw_fixture()
    step_fixture()
    elementwise_fixture()
    bottleneck_fixture("bottleneck3d_se_ds", 16, 8, 2, 3, 0, True, (2, 16, 4, 12, 12), 31)
    bottleneck_fixture("bottleneck3d_plain", 32, 8, 1, 1, 1, False, (3, 32, 3, 8, 8), 32)
    slowfast_fixture()
    gb_loops_fixture()
    cnnlstm_fixture()
    mlstm_fcn_fixture()
    transformer0d_fixture()
    vivit_fixture()
    multimodal_fixture()
    fusion_derived_fixture()
