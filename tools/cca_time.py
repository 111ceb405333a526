#!/usr/bin/env python3
"""Time the Deep-CCA loss on the GPU and print one JSON line (also written to --out).

Per (m, o) in {(64, 128), (256, 64), (512, 128)} and mode (top-k with k = 10, all singular values): ms per ``CCALoss`` forward plus
backward (median of --iters device-event intervals after --warmup calls), the launches per call (counted from the library's own
fixed chain: 9 forward + 9 backward), the Jacobi sweeps the three eigenproblems took, and beside it the same loss composed from
``torch.linalg.eigh`` in float32 on the same GPU with autograd (its gradient divides by eigenvalue gaps; the figure is a time, not an
accuracy statement), with a note on whether that composition could be captured in a HIP graph (tried in a child process).  ``md_sym_eig`` alone at n = 32, 64 and
128 (one matrix, and the loss's batch of two), against ``torch.linalg.eigh`` on the same matrices.
Usage: python tools/cca_time.py [--iters 200] [--warmup 20] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "disruption-prediciton-based-on-multimodal-deep-learning_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

FWD_LAUNCHES, BWD_LAUNCHES = 9, 9         # csrc/cca.hip: md_cca_loss_fwd / md_cca_loss_bwd


def events(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return round(statistics.median(ms), 4), round(min(ms), 4)


def planted(m, o, seed):
    rng = np.random.default_rng(seed)
    z, e = rng.standard_normal((m, o)), rng.standard_normal((m, o))
    rho = np.linspace(.98, .02, o)
    a, b = rng.standard_normal((o, o)) / o ** 0.5, rng.standard_normal((o, o)) / o ** 0.5
    return (z @ a + 0.3).astype(np.float32), ((z * rho + e * np.sqrt(1 - rho * rho)) @ b - 0.2).astype(np.float32)


def torch_loss(h1, h2, k, use_all, r=1e-3, eps=1e-6):
    """The same loss from torch.linalg.eigh and autograd (float32)."""
    m, o1 = h1.shape
    o2 = h2.shape[1]
    H1, H2 = (h1 - h1.mean(0, keepdim=True)).t(), (h2 - h2.mean(0, keepdim=True)).t()
    S12 = H1 @ H2.t() / (m - 1)
    S11 = H1 @ H1.t() / (m - 1) + r * torch.eye(o1, device=h1.device)
    S22 = H2 @ H2.t() / (m - 1) + r * torch.eye(o2, device=h1.device)
    d1, V1 = torch.linalg.eigh(S11)
    d2, V2 = torch.linalg.eigh(S22)
    T = (V1 * d1.clamp_min(eps).rsqrt()) @ V1.t() @ S12 @ (V2 * d2.clamp_min(eps).rsqrt()) @ V2.t()
    lam = torch.linalg.eigvalsh(T.t() @ T + (0.0 if use_all else r) * torch.eye(o2, device=h1.device))
    lam = lam.clamp_min(0.0 if use_all else eps)
    return -(lam if use_all else lam.topk(k)[0]).sqrt().sum()


def capture(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def probe_torch_capture():
    """Child process: can the torch.linalg.eigh composition be captured?  Prints one line.  A failed capture can leave the runtime
    in an error state, so the attempt gets a process of its own."""
    dev = torch.device("cuda:0")
    n1, n2 = planted(256, 64, 1)
    a, b = torch.from_numpy(n1).to(dev).requires_grad_(), torch.from_numpy(n2).to(dev).requires_grad_()
    try:
        capture(lambda: torch.autograd.grad(torch_loss(a, b, 10, False), (a, b)))
        print("captured")
    except Exception as e:                                        # noqa: BLE001
        print("not capturable: " + (str(e).strip().splitlines() or [type(e).__name__])[0][:200])


def torch_capture_verdict():
    try:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--probe-torch-capture"], capture_output=True, text=True,
                             timeout=180)
    except subprocess.TimeoutExpired:
        return "not capturable: the attempt did not finish in 180 s"
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith(("captured", "not capturable"))]
    return lines[-1] if lines else "not capturable: the attempt ended the process (exit code %d)" % out.returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--probe-torch-capture", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cca_time: needs the GPU (a time taken elsewhere says nothing)")
    if args.probe_torch_capture:
        return probe_torch_capture()
    from src import CCA, ops
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup, "loss": [], "sym_eig": []}
    for m, o in ((64, 128), (256, 64), (512, 128)):
        n1, n2 = planted(m, o, m + o)
        for use_all in (False, True):
            a, b = torch.from_numpy(n1).to(dev).requires_grad_(), torch.from_numpy(n2).to(dev).requires_grad_()
            fn = CCA.CCALoss(10, use_all)

            def ours():
                return torch.autograd.grad(fn(a, b), (a, b))

            def theirs():
                return torch.autograd.grad(torch_loss(a, b, 10, use_all), (a, b))
            med, best = events(ours, args.iters, args.warmup)
            _, ws = ops.cca_loss_fwd(a.detach(), b.detach(), 0 if use_all else 10, 1e-3, 1e-3, 1e-6)
            sweeps = ops.cca_workspace_view(ws, m, o, o, "sweeps").cpu().tolist()
            graph = capture(ours)
            gmed, _ = events(graph.replay, args.iters, args.warmup)
            tmed, tbest = events(theirs, args.iters, args.warmup)
            l_ours, l_torch = float(fn(a, b).detach()), float(torch_loss(a, b, 10, use_all).detach())
            res["loss"].append({"m": m, "o": o, "mode": "all" if use_all else "top10", "ms_fwd_bwd": med, "ms_min": best,
                                "ms_graph_replay": gmed, "launches": FWD_LAUNCHES + BWD_LAUNCHES, "sweeps_s11_s22_tt": sweeps,
                                "loss": l_ours, "torch_eigh_ms_fwd_bwd": tmed, "torch_eigh_ms_min": tbest, "torch_eigh_loss": l_torch})
    for n in (32, 64, 128):
        rng = np.random.default_rng(n)
        x = rng.standard_normal((2, n, 2 * n))
        mats = torch.from_numpy((x @ x.transpose(0, 2, 1) / (2 * n)).astype(np.float32)).to(dev)
        one = mats[0].contiguous()
        m1, _ = events(lambda: ops.sym_eig(one), args.iters, args.warmup)
        m2, _ = events(lambda: ops.sym_eig(mats), args.iters, args.warmup)
        t1, _ = events(lambda: torch.linalg.eigh(one), args.iters, args.warmup)
        t2, _ = events(lambda: torch.linalg.eigh(mats), args.iters, args.warmup)
        res["sym_eig"].append({"n": n, "ms_one": m1, "ms_batch2": m2, "sweeps": ops.sym_eig(mats)[2].cpu().tolist(),
                               "torch_eigh_ms_one": t1, "torch_eigh_ms_batch2": t2})
    res["torch_eigh_graph"] = torch_capture_verdict()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
