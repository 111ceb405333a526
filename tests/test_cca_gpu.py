"""GPU tests of Deep CCA (csrc/cca.hip, src/CCA.py): the LDS eigensolver alone against LAPACK, the loss and its closed-form gradient
against the recordings of tests/golden/cca_loss*.npz (reference autograd in float64), input handling, HIP graph capture, train_cca
against the reference's recorded run, and one step through the real encoders.

Bars.  Eigensolver: 10 x what numpy.linalg.eigh (LAPACK, float32) attains on the same matrix, computed in the test, floor 1e-6 on the
residual and the orthogonality.  Loss and gradients: 10 x the recorded ``self32`` figure (the float32 run of tests/cca_util.py), floors
1e-6 relative on the loss and 1e-5 relative L2 on a gradient.  Every figure is printed before it is asserted (pytest -s)."""
import os

import numpy as np
import pytest
import torch

from src import CCA, ops
from tests import cca_util as cu

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def gpu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = dict(np.load(os.path.join(golden_dir, "cca_loss.npz")))
    g.update(np.load(os.path.join(golden_dir, "cca_loss_E.npz")))
    return g


# ------------------------------------------------------------------------------------------------------------------ md_sym_eig
def _g_cov(ridge):
    out = []
    for h in cu.case_inputs("G"):
        H = (h - h.mean(0)).astype(np.float64)
        out.append((H.T @ H / (len(h) - 1) + ridge * np.eye(h.shape[1])).astype(np.float32))
    return np.stack(out)


def eig_inputs(kind, n):
    rng = np.random.default_rng(100 * n + len(kind))
    if kind == "spd":
        xs = [rng.standard_normal((n, 2 * n + 3)) for _ in range(2)]
        return np.stack([x @ x.T / (2 * n + 3) for x in xs]).astype(np.float32)
    if kind == "diag":
        return np.stack([np.diag(rng.standard_normal(n)) for _ in range(2)]).astype(np.float32)
    if kind == "zero":
        return np.zeros((2, n, n), np.float32)
    if kind == "rank1":                                           # I + u u^T: an (n-1)-fold eigenvalue
        us = [rng.standard_normal((n, 1)) for _ in range(2)]
        return np.stack([np.eye(n) + u @ u.T for u in us]).astype(np.float32)
    raise KeyError(kind)


EIG_CASES = [(k, n) for n in (1, 2, 5, 33, 64, 128) for k in ("spd", "diag", "zero", "rank1")] + [("g_s11", 16), ("g_s11_1e6", 16)]


def _figures(a, w, v):
    a64 = a.astype(np.float64)
    v64 = v.astype(np.float64)
    nrm = max(np.linalg.norm(a64), 1e-300)
    res = np.linalg.norm(a64 @ v64 - v64 * w.astype(np.float64)) / nrm
    orth = np.abs(v64.T @ v64 - np.eye(len(w))).max()
    w64 = np.linalg.eigvalsh(a64)
    werr = np.abs(w.astype(np.float64) - w64).max() / max(np.abs(w64).max(), 1e-300)
    return res, orth, werr


@pytest.mark.parametrize("kind,n", EIG_CASES)
def test_sym_eig_against_lapack(kind, n):
    if kind.startswith("g_s11"):
        a = _g_cov(1e-6 if kind.endswith("1e6") else cu.R1)
        if kind.endswith("1e6"):
            assert np.linalg.cond(a[0].astype(np.float64)) >= 1e6
    else:
        a = eig_inputs(kind, n)
    assert a.shape == (2, n, n) and (kind == "zero" or not np.array_equal(a[0], a[1]))
    d = gpu(a)
    w, v, sweeps = ops.sym_eig(d)
    w2, v2, sweeps2 = ops.sym_eig(d)
    assert torch.equal(w, w2) and torch.equal(v, v2) and torch.equal(sweeps, sweeps2)          # the same input gives the same bits
    w, v, sweeps = w.cpu().numpy(), v.cpu().numpy(), sweeps.cpu().numpy()
    for b in range(2):
        mine = _figures(a[b], w[b], v[b])
        lap = _figures(a[b], *np.linalg.eigh(a[b]))
        print("sym_eig %-9s n %3d [%d] sweeps %2d | residual %.2e (LAPACK %.2e) orthogonality %.2e (%.2e) eigenvalues %.2e (%.2e)" % (
            kind, n, b, sweeps[b], mine[0], lap[0], mine[1], lap[1], mine[2], lap[2]))
        assert np.all(np.isfinite(w[b])) and np.all(np.isfinite(v[b]))
        assert mine[0] <= max(10 * lap[0], 1e-6)
        assert mine[1] <= max(10 * lap[1], 1e-6)
        assert np.all(np.diff(w[b]) >= 0)
        assert mine[2] <= 10 * lap[2]
        top = np.argmax(np.abs(v[b]), axis=0)                     # first row of the largest magnitude in every column
        assert np.all(v[b][top, np.arange(n)] > 0)
        assert 1 <= sweeps[b] < 30
    single = ops.sym_eig(d[1])                                    # (n, n) input: the same kernel on one matrix
    assert torch.equal(single[0], w2[1]) and torch.equal(single[1], v2[1])


def test_sym_eig_refuses_large_and_cpu_input():
    with pytest.raises(ValueError, match="128"):
        ops.sym_eig(torch.zeros(129, 129, device=DEV))
    with pytest.raises(RuntimeError):
        ops.sym_eig(torch.zeros(4, 4))


# ------------------------------------------------------------------------------------------------------------------ loss, gradients
_RUNS = {}


def run_loss(h1, h2, k, use_all, scale=None):
    a, b = gpu(h1).requires_grad_(), gpu(h2).requires_grad_()
    loss = CCA.CCALoss(k, use_all)(a, b)
    (loss if scale is None else scale * loss).backward()
    return float(loss.detach()), a.grad.cpu().numpy(), b.grad.cpu().numpy()


def case_run(golden, case, mode):
    key = (case, mode)
    if key not in _RUNS:
        _RUNS[key] = run_loss(golden["h1/" + case], golden["h2/" + case], cu.CASES[case][2], mode == "all")
    return _RUNS[key]


def bar(golden, key, floor):
    return max(10.0 * float(golden["self32/" + key]), floor)


@pytest.mark.parametrize("mode", ["topk", "all"])
@pytest.mark.parametrize("case", ["A", "B", "C", "D", "E", "F"])
def test_loss_and_gradients_against_the_reference(golden, case, mode):
    loss, g1, g2 = case_run(golden, case, mode)
    key = "%s/loss/%s" % (mode, case)
    dev = cu.rel_abs(loss, golden[key])
    print("cca %s: loss deviation %.2e (bar %.2e)" % (key, dev, bar(golden, key, 1e-6)))
    assert dev <= bar(golden, key, 1e-6)
    assert np.all(np.isfinite(g1)) and np.all(np.isfinite(g2))
    checked = 0
    for name, mine in (("g1", g1), ("g2", g2)):
        key = "%s/%s/%s" % (mode, name, case)
        if key in golden:
            dev = cu.rel_l2(mine, golden[key])
            print("cca %s: gradient deviation %.2e (bar %.2e)" % (key, dev, bar(golden, key, 1e-5)))
            assert dev <= bar(golden, key, 1e-5)
            checked += 1
    assert checked == (2 if case in (cu.TOPK_GRAD if mode == "topk" else cu.ALL_GRAD) else 0)


@pytest.mark.parametrize("mode", ["topk", "all"])
def test_degenerate_case_g_loss_and_finite_gradients(golden, mode):
    loss, g1, g2 = case_run(golden, "G", mode)
    key = "%s/loss/G" % mode
    dev = cu.rel_abs(loss, golden[key])
    print("cca %s: loss deviation %.2e (bar %.2e)" % (key, dev, bar(golden, key, 1e-6)))
    assert dev <= bar(golden, key, 1e-6)
    assert np.all(np.isfinite(g1)) and np.all(np.isfinite(g2))


@pytest.mark.parametrize("k,use_all", [(3, False), (0, True)])
def test_unequal_widths(k, use_all):
    rng = np.random.default_rng(3)
    h1, h2 = rng.standard_normal((30, 12)).astype(np.float32), rng.standard_normal((30, 7)).astype(np.float32)
    want = cu.cca_closed_form(h1, h2, k, use_all)
    f32 = cu.cca_closed_form(h1, h2, k, use_all, np.float32)
    got = run_loss(h1, h2, k if k else 5, use_all)
    bars = (max(10 * cu.rel_abs(f32[0], want[0]), 1e-6), max(10 * cu.rel_l2(f32[1], want[1]), 1e-5), max(10 * cu.rel_l2(f32[2], want[2]), 1e-5))
    devs = (cu.rel_abs(got[0], want[0]), cu.rel_l2(got[1], want[1]), cu.rel_l2(got[2], want[2]))
    print("cca unequal widths (30, 12, 7) k %d: loss %.2e (bar %.2e) g1 %.2e (%.2e) g2 %.2e (%.2e)" % (
        k, devs[0], bars[0], devs[1], bars[1], devs[2], bars[2]))
    assert got[1].shape == (30, 12) and got[2].shape == (30, 7)
    assert all(d <= b for d, b in zip(devs, bars))


def test_non_contiguous_input_and_incoming_gradient(golden):
    h1, h2 = golden["h1/B"], golden["h2/B"]
    plain = case_run(golden, "B", "topk")
    a = gpu(h1.T.copy()).requires_grad_()                         # (o, m) storage; the loss sees its transposed view
    b = gpu(h2).requires_grad_()
    assert not a.t().is_contiguous()
    loss = CCA.CCALoss(4, False)(a.t(), b)
    (2.5 * loss).backward()
    assert float(loss) == plain[0]
    d1, d2 = cu.rel_l2(a.grad.t().cpu().numpy() / 2.5, plain[1]), cu.rel_l2(b.grad.cpu().numpy() / 2.5, plain[2])
    print("cca incoming gradient 2.5: deviation from 2.5 x the plain gradient %.2e %.2e" % (d1, d2))
    assert d1 <= 1e-6 and d2 <= 1e-6
    key = "topk/g1/B"
    assert cu.rel_l2(a.grad.t().cpu().numpy() / 2.5, golden[key]) <= bar(golden, key, 1e-5)


def test_argument_checks_on_the_device():
    z = torch.zeros(8, 4, device=DEV)
    with pytest.raises(ValueError, match="128"):
        CCA.CCALoss(2, False)(torch.zeros(8, 129, device=DEV), z)
    with pytest.raises(ValueError, match="128"):
        CCA.CCALoss(2, True)(z, torch.zeros(8, 640, device=DEV))
    with pytest.raises(ValueError, match="output_dim"):
        CCA.CCALoss(5, False)(torch.zeros(8, 6, device=DEV), z)
    with pytest.raises(RuntimeError):
        CCA.CCALoss(2, False)(z, torch.zeros(8, 4))
    assert torch.isfinite(CCA.CCALoss(5, True)(torch.randn(8, 6, device=DEV), torch.randn(8, 4, device=DEV)))   # output_dim unused with all values


@pytest.mark.parametrize("use_all", [False, True])
def test_forward_and_backward_in_one_hip_graph(golden, use_all):
    fn = CCA.CCALoss(6, use_all)
    a, b = gpu(golden["h1/C"]).requires_grad_(), gpu(golden["h2/C"]).requires_grad_()

    def step():
        loss = fn(a, b)
        g1, g2 = torch.autograd.grad(loss, (a, b))
        return loss.detach(), g1, g2     # nothing that is kept holds an autograd graph (a stale one breaks the capture)
    eager = [t.clone() for t in step()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for t in out:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(out, eager))
    with torch.no_grad():                                         # new values in the captured inputs: the replay follows them
        a.copy_(gpu(golden["h1/C"][::-1].copy()))
        b.copy_(gpu(golden["h2/C"][::-1].copy()))
    graph.replay()
    torch.cuda.synchronize()
    assert abs(float(out[0]) - float(eager[0])) <= 1e-5 * abs(float(eager[0]))         # the rows in another order: the same loss
    assert all(torch.equal(x, y) for x, y in zip(out, step()))


# ------------------------------------------------------------------------------------------------------------------ training
def test_train_cca_end_to_end_against_the_reference_run(golden_dir, tmp_path, capsys):
    g = np.load(os.path.join(golden_dir, "cca_train.npz"))
    train, valid = cu.train_setup()
    model = CCA.DeepCCA(torch.nn.Linear(12, 6), torch.nn.Linear(9, 6))
    model.load_state_dict({k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd/")}, strict=True)
    opt = torch.optim.SGD(model.parameters(), lr=1e-2)
    tl, vl = CCA.train_cca(train, valid, model, opt, None, CCA.CCALoss(3, False), "cuda:0", 3, None,
                           str(tmp_path / "best.pt"), str(tmp_path / "last.pt"), None)
    out = capsys.readouterr().out
    assert "x1 : " not in out and "loss : tensor" not in out
    dt = np.max(np.abs(np.array(tl) - g["train_loss"]) / np.abs(g["train_loss"]))
    dv = np.max(np.abs(np.array(vl) - g["valid_loss"]) / np.abs(g["valid_loss"]))
    print("train_cca: per-epoch deviation from the reference's float64 run: train %.2e valid %.2e (bar 1e-4)" % (dt, dv))
    print("train_cca: losses", tl, vl)
    assert dt <= 1e-4 and dv <= 1e-4
    assert tl[2] < tl[0] and os.path.exists(tmp_path / "best.pt") and os.path.exists(tmp_path / "last.pt")
    assert abs(CCA.evaluate_cca_loss(valid, model, CCA.CCALoss(3, False), "cuda:0") - vl[2]) <= 1e-6 * abs(vl[2])


def test_real_encoders_one_step():
    from src.models.ViViT import ViViTEncoder
    from src.models.transformer import TransformerEncoder
    torch.manual_seed(5)
    model = CCA.DeepCCA(ViViTEncoder(image_size=32, patch_size=8, n_frames=5, dim=8, depth=1, n_heads=2, d_head=8, scale_dim=2),
                        TransformerEncoder(n_features=6, kernel_size=3, feature_dims=8, max_len=5, n_layers=1, n_heads=2,
                                           dim_feedforward=16, dropout=0.0)).to(DEV)
    model.train()
    clip, sig = torch.randn(24, 3, 5, 32, 32, device=DEV), torch.randn(24, 5, 6, device=DEV)
    fn = CCA.CCALoss(3, False)
    opt = torch.optim.SGD(model.parameters(), lr=0.05)
    z1, z2 = model(clip, sig)
    assert z1.shape == (24, 8) and z2.shape == (24, 8)
    loss = fn(z1, z2)
    loss.backward()
    for enc in (model.encoder_1, model.encoder_2):
        grads = [p.grad for p in enc.parameters() if p.grad is not None]
        assert grads and all(torch.isfinite(x).all() for x in grads) and any(float(x.abs().max()) > 0 for x in grads)
    opt.step()
    with torch.no_grad():
        after = fn(*model(clip, sig))
    print("real encoders: loss %.6f -> %.6f" % (float(loss), float(after)))
    assert torch.isfinite(after) and float(after) != float(loss)
