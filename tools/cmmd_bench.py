"""Two readings of the CMMD path on the HIP kernels (no gate: there is no earlier path to compare with).

(a) ``uspace_metric_rbf_sums`` alone on synthetic embedding banks of width 768, normalised, sigma = 10, at 50 000 x 50 000 and at
    5 000 x 30 000: wall time (HIP events, after a warm-up) and the fp64 FLOP/s of the Gram part (2 F per pair of every tile
    computed: nx^2 + ny^2 + nx ny pairs, both triangles of the symmetric blocks; the exp and the sums are not counted).  For
    context the same three sums by chunked fp64 ``torch`` matmul + exp on the same box, and the ratio of the two times.
(b) ``CMMD.update`` from 256^2 samples with the seeded CLIP ViT-L/14-336 tower (577 tokens, 24 layers), preprocess included:
    images/s at batch 16 and 64.
Also the box's device-to-device copy bandwidth (1 GiB, read + write counted), to tell a slow box from a slow kernel.
Prints one JSON line; the reading is kept in profiles/cmmd.md.
    python tools/cmmd_bench.py [--iters 3] [--reps 3] [--skip-tower]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

FP64_MATRIX_PEAK_TF = 78.6        # MI355X data sheet, fp64 matrix
SIGMA = 10.0


def timed_ms(fn, iters, reps, warmup=1):
    """ms per call: median and (min, max) over ``reps`` event-timed windows of ``iters`` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return statistics.median(out), min(out), max(out)


def synthetic(n, F, seed, shift):
    """Embedding-like banks: a common direction plus a low-dimensional spread, so that the normalised kernel values sit near 1."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    lat = torch.randn(n, 16, generator=g, device="cuda")
    basis = torch.randn(16, F, generator=g, device="cuda") / 4
    return (lat @ basis + 0.05 * torch.randn(n, F, generator=g, device="cuda") + 1.0 + shift).contiguous()


def torch_sums(x, y, gamma, chunk=4096):
    """The same three sums by fp64 torch: rows normalised, chunks of rows against the whole other set, the diagonal subtracted."""
    xd, yd = (torch.nn.functional.normalize(t.double(), dim=1) for t in (x, y))
    out = []
    for a, b, off in ((xd, xd, True), (yd, yd, True), (xd, yd, False)):
        s = torch.zeros((), dtype=torch.float64, device=x.device)
        for lo in range(0, a.shape[0], chunk):
            d2 = (2.0 - 2.0 * (a[lo:lo + chunk] @ b.T)).clamp_(min=0.0)
            s += torch.exp_(d2.mul_(-gamma)).sum()
        out.append(s - (a.shape[0] if off else 0))
    return torch.stack(out)


def copy_gb_per_s():
    a = torch.empty(1 << 28, dtype=torch.float32, device="cuda")
    b = torch.empty_like(a)
    ms = timed_ms(lambda: b.copy_(a), 10, 3)[0]
    return 2.0 * a.numel() * 4 / (ms * 1e-3) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dims", type=int, default=768)
    ap.add_argument("--skip-tower", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "cmmd_bench needs a ROCm device"
    from uspace_amd import _hip
    from uspace_amd.libs.clip import CLIP_L_336_VISION, CLIPVisionTransformer
    from uspace_amd.tools.cmmd import CMMD, mmd2_from_sums
    F, gamma = a.dims, 1.0 / (2.0 * SIGMA * SIGMA)
    res = {"workload": "uspace_metric_rbf_sums (normalised, sigma 10) and CMMD.update with the CLIP ViT-L/14-336 tower, seeded weights",
           "F": F, "fp64_matrix_peak_tflops": FP64_MATRIX_PEAK_TF, "iters": a.iters, "reps": a.reps, "copy_gb_per_s": copy_gb_per_s()}
    for nx, ny in ((50000, 50000), (5000, 30000)):
        x, y = synthetic(nx, F, 1, 0.0), synthetic(ny, F, 2, 0.02)
        ws = _hip.metric_workspace(nx, ny, 1, max(nx, ny), device=x.device)
        ms = timed_ms(lambda: _hip.metric_rbf_sums(x, y, gamma, normalize=True, ws=ws), a.iters, a.reps)
        ms_t = timed_ms(lambda: torch_sums(x, y, gamma), 1, a.reps)
        sums, sums_t = _hip.metric_rbf_sums(x, y, gamma, normalize=True, ws=ws).cpu(), torch_sums(x, y, gamma).cpu()
        flop = 2.0 * F * (float(nx) * nx + float(ny) * ny + float(nx) * ny)
        tf = flop / (ms[0] * 1e-3) / 1e12
        res[f"rbf_{nx}x{ny}"] = {"ms": ms[0], "ms_min_max": ms[1:], "gram_fp64_tflops": tf, "frac_of_peak": tf / FP64_MATRIX_PEAK_TF,
                                 "torch_fp64_ms": ms_t[0], "torch_fp64_ms_min_max": ms_t[1:], "torch_over_hip": ms_t[0] / ms[0],
                                 "cmmd": 1000.0 * mmd2_from_sums(sums.tolist(), nx, ny),
                                 "cmmd_torch_fp64": 1000.0 * mmd2_from_sums(sums_t.tolist(), nx, ny)}
        del x, y, ws
    if not a.skip_tower:
        torch.manual_seed(0)
        metric = CMMD(CLIPVisionTransformer(**CLIP_L_336_VISION), device="cuda")
        g = torch.Generator().manual_seed(1)
        for B in (16, 64):
            imgs = torch.rand(B, 3, 256, 256, generator=g).cuda()

            def update():
                metric.reset(real=False)
                metric.update(imgs)

            ms = timed_ms(update, a.iters, a.reps, warmup=2)
            res[f"update_b{B}"] = {"ms": ms[0], "ms_min_max": ms[1:], "img_per_s": B / ms[0] * 1e3}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
