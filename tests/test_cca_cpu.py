"""CPU tests of Deep CCA: the float64 closed form of tests/cca_util.py (what tests/test_cca_gpu.py compares the kernels with) against
the recordings of tests/golden/cca_loss*.npz (written by tests/golden/make_cca_golden.py from autograd through the reference's own
CCALoss), the host logic of the training loops on a stub loss, and the argument checks of the C ABI and of CCALoss."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from src import CCA, _native
from tests import cca_util as cu


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = dict(np.load(os.path.join(golden_dir, "cca_loss.npz")))
    g.update(np.load(os.path.join(golden_dir, "cca_loss_E.npz")))
    return g


@pytest.mark.parametrize("case", sorted(cu.CASES))
def test_closed_form_reproduces_the_reference_autograd(golden, case):
    m, o, k, rho = cu.CASES[case]
    h1, h2 = golden["h1/" + case], golden["h2/" + case]
    assert h1.dtype == np.float32 and h1.shape == (int(golden["rows/E"]) if case == "E" else m, o)
    gen1, gen2 = cu.planted(h1.shape[0], o, rho)
    assert np.array_equal(gen1, h1) and np.array_equal(gen2, h2)            # the seeded recipe still gives the recorded inputs
    for mode, use_all in (("topk", False), ("all", True)):
        loss, g1, g2, sv = cu.cca_closed_form(h1, h2, k, use_all)
        assert cu.rel_abs(loss, golden["%s/loss/%s" % (mode, case)]) <= 1e-7
        for name, mine in (("g1", g1), ("g2", g2)):
            key = "%s/%s/%s" % (mode, name, case)
            if key in golden:
                dev = cu.rel_l2(mine, golden[key])
                print(key, "closed form vs recording", dev)
                assert dev <= 1e-7
        assert np.allclose(sv, golden["sv/" + case], rtol=0, atol=1e-9)
    assert ("topk/g1/" + case in golden) == (case in cu.TOPK_GRAD) and ("all/g1/" + case in golden) == (case in cu.ALL_GRAD)


def test_recorded_conditions_hold(golden):
    for case in cu.TOPK_GRAD:
        k, sv = cu.CASES[case][2], golden["sv/" + case]
        assert sv[k - 1] - sv[k] >= 2e-3
    for case in cu.ALL_GRAD:
        assert golden["sv/" + case].min() >= 1e-2


def test_all_values_loss_is_the_nuclear_norm(golden):
    h1, h2 = golden["h1/C"], golden["h2/C"]
    loss, _, _, sv = cu.cca_closed_form(h1, h2, 6, True)
    assert abs(loss + sv.sum()) <= 1e-9 * sv.sum()


def test_unequal_widths_against_autograd():
    rng = np.random.default_rng(3)
    h1, h2 = rng.standard_normal((30, 12)), rng.standard_normal((30, 7))
    for k, use_all in ((3, False), (0, True)):
        a, b = torch.from_numpy(h1).requires_grad_(), torch.from_numpy(h2).requires_grad_()
        H1, H2 = (a - a.mean(0)).t(), (b - b.mean(0)).t()
        S12 = H1 @ H2.t() / 29
        S11, S22 = H1 @ H1.t() / 29 + cu.R1 * torch.eye(12, dtype=torch.float64), H2 @ H2.t() / 29 + cu.R2 * torch.eye(7, dtype=torch.float64)

        def isq(S):
            d, V = torch.linalg.eigh(S)
            return V @ torch.diag(d ** -0.5) @ V.t()
        T = isq(S11) @ S12 @ isq(S22)
        sv = torch.linalg.svdvals(T)
        loss = -(sv.sum() if use_all else torch.sqrt(sv[:k] ** 2 + cu.R1).sum())
        loss.backward()
        mine = cu.cca_closed_form(h1, h2, k, use_all)
        assert cu.rel_abs(mine[0], loss.item()) <= 1e-9
        assert cu.rel_l2(mine[1], a.grad.numpy()) <= 1e-7 and cu.rel_l2(mine[2], b.grad.numpy()) <= 1e-7


# ---------------------------------------------------------------------------------------------------------- host logic on a stub
class _StubLoss(torch.nn.Module):
    def forward(self, z1, z2):
        return ((z1 - z2) ** 2).mean()


def test_train_cca_host_logic_on_a_stub(tmp_path, capsys):
    torch.manual_seed(0)
    train, valid = cu.train_setup()
    train = [({"video": d["video"][:, :9], "0D": d["0D"]}, t) for d, t in train]
    valid = [({"video": d["video"][:, :9], "0D": d["0D"]}, t) for d, t in valid]
    model = CCA.DeepCCA(torch.nn.Linear(9, 4), torch.nn.Linear(9, 4))
    twin = CCA.DeepCCA(torch.nn.Linear(9, 4), torch.nn.Linear(9, 4))
    twin.load_state_dict(model.state_dict())
    opt = torch.optim.SGD(model.parameters(), lr=0.05)
    sched = torch.optim.lr_scheduler.StepLR(opt, 1, 0.5)
    best, last = str(tmp_path / "best.pt"), str(tmp_path / "last.pt")
    tl, vl = CCA.train_cca(train, valid, model, opt, sched, _StubLoss(), "cpu", 3, 2, best, last, 0.25)
    out = capsys.readouterr().out
    assert out.count("\nepoch : ") + out.startswith("epoch : ") == 2 and "x1 : " not in out and "(Report)" in out       # verbose = 2: epochs 1 and 3; no debug prints
    # the same three epochs written out by hand: clipping, one scheduler step per epoch, mean over the batches
    opt2 = torch.optim.SGD(twin.parameters(), lr=0.05)
    want_t, want_v, lr = [], [], 0.05
    for epoch in range(3):
        for g in opt2.param_groups:
            g["lr"] = lr
        acc = 0.0
        for d, _ in train:
            opt2.zero_grad()
            loss = _StubLoss()(*twin(d["video"], d["0D"]))
            loss.backward()
            torch.nn.utils.clip_grad_norm_(twin.parameters(), 0.25)
            opt2.step()
            acc += loss.item()
        lr *= 0.5
        want_t.append(acc / len(train))
        with torch.no_grad():
            want_v.append(sum(_StubLoss()(*twin(d["video"], d["0D"])).item() for d, _ in valid) / len(valid))
    assert np.allclose(tl, want_t, rtol=1e-6) and np.allclose(vl, want_v, rtol=1e-6)
    assert isinstance(tl, list) and isinstance(tl[0], float) and len(vl) == 3
    saved_last, saved_best = torch.load(last), torch.load(best)
    for k_, v_ in model.state_dict().items():
        assert torch.equal(saved_last[k_], v_)
    assert vl[2] == min(vl) and all(torch.equal(saved_best[k_], v_) for k_, v_ in model.state_dict().items())
    assert abs(CCA.evaluate_cca_loss(valid, model, _StubLoss(), "cpu") - vl[2]) <= 1e-7


def test_deepcca_forward_returns_both_latents():
    model = CCA.DeepCCA(torch.nn.Linear(5, 3), torch.nn.Linear(4, 2))
    z1, z2 = model(torch.ones(6, 5), torch.ones(6, 4))
    assert z1.shape == (6, 3) and z2.shape == (6, 2)


# ---------------------------------------------------------------------------------------------------------- argument checks
def test_cca_loss_refuses_cpu_tensors_and_bad_widths():
    loss = CCA.CCALoss(2, False)
    assert (loss.r1, loss.r2, loss.eps) == (1e-3, 1e-3, 1e-6)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        loss(torch.zeros(8, 4), torch.zeros(8, 4))


def test_cca_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _native.lib()
    a = C.c_void_p(64)                                             # a non-null pointer that is never dereferenced: every call is refused
    NULL, SHAPE, UNSUP = -5, -1, -2
    assert lib.md_sym_eig(None, 1, 4, a, a, None, None) == NULL and lib.md_sym_eig(a, 1, 4, None, a, None, None) == NULL
    assert lib.md_sym_eig(a, 1, 4, a, None, None, None) == NULL
    assert lib.md_sym_eig(a, 1, 0, a, a, None, None) == SHAPE and lib.md_sym_eig(a, 0, 4, a, a, None, None) == SHAPE
    assert lib.md_sym_eig(a, 1, 129, a, a, None, None) == UNSUP
    fwd = lambda h1, h2, m, o1, o2, k, ws, loss: lib.md_cca_loss_fwd(h1, h2, m, o1, o2, k, 1e-3, 1e-3, 1e-6, ws, loss, None)   # noqa: E731
    assert fwd(None, a, 8, 4, 4, 2, a, a) == NULL and fwd(a, None, 8, 4, 4, 2, a, a) == NULL
    assert fwd(a, a, 8, 4, 4, 2, None, a) == NULL and fwd(a, a, 8, 4, 4, 2, a, None) == NULL
    assert fwd(a, a, 1, 4, 4, 2, a, a) == SHAPE and fwd(a, a, 8, 0, 4, 2, a, a) == SHAPE
    assert fwd(a, a, 8, 4, 3, 4, a, a) == SHAPE and fwd(a, a, 8, 4, 4, -1, a, a) == SHAPE        # k > o2, k < 0
    assert fwd(a, a, 8, 129, 4, 2, a, a) == UNSUP and fwd(a, a, 8, 4, 129, 2, a, a) == UNSUP
    bwd = lambda g, m, o1, o2, k, ws, d1, d2: lib.md_cca_loss_bwd(g, m, o1, o2, k, 1e-6, ws, d1, d2, None)                  # noqa: E731
    assert bwd(None, 8, 4, 4, 2, a, a, a) == NULL and bwd(a, 8, 4, 4, 2, None, a, a) == NULL
    assert bwd(a, 8, 4, 4, 2, a, None, a) == NULL and bwd(a, 8, 4, 4, 2, a, a, None) == NULL
    assert bwd(a, 1, 4, 4, 2, a, a, a) == SHAPE and bwd(a, 8, 4, 3, 4, a, a, a) == SHAPE and bwd(a, 8, 4, 129, 2, a, a, a) == UNSUP
    assert lib.md_cca_workspace_floats(1, 4, 4) == 0 and lib.md_cca_workspace_floats(8, 129, 4) == 0
    assert lib.md_cca_workspace_floats(8, 4, 4) >= 2 * 8 * 4 + 20 * 16
    n = lib.md_cca_workspace_floats(512, 128, 128)
    offs = [lib.md_cca_workspace_offset(512, 128, 128, w) for w in range(5)]
    assert all(0 <= o < n for o in offs) and len(set(offs)) == 5 and lib.md_cca_workspace_offset(512, 128, 128, 5) == -1
