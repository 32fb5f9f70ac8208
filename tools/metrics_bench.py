"""Wall time of the feature-set metrics on the HIP kernels: ``prdc`` (nearest_k = 5) and ``kid_score`` (100 subsets of 1000) on
synthetic banks at N = M = 10 000 and 50 000, F = 2 048, timed with HIP events after a warm-up, with the fp64 FLOP/s the Gram
kernels achieved next to the time (2 F multiply-adds' worth per pair of every tile computed: N^2 + M^2 + 2 N M pairs for prdc,
3 m^2 per subset for KID -- both triangles of the symmetric blocks are computed and counted).  No gate: there is nothing to
compare with.  Prints one JSON line; the reading is kept in profiles/feature_metrics.md.
    python tools/metrics_bench.py [--sizes 10000 50000] [--iters 2]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

FP64_MATRIX_PEAK_TF = 78.6        # MI355X data sheet, fp64 matrix


def timed_ms(fn, iters):
    fn()                                           # warm-up
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def synthetic(n, F, seed, shift):
    """Features with the structure of pool features: non-negative, a common offset, a low-dimensional spread."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    lat = torch.randn(n, 16, generator=g, device="cuda")
    basis = torch.randn(16, F, generator=g, device="cuda") / 4
    return (lat @ basis + 0.05 * torch.randn(n, F, generator=g, device="cuda") + 1.0 + shift).clamp_(min=0).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[10000, 50000])
    ap.add_argument("--dims", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "metrics_bench needs a ROCm device"
    from uspace_amd.tools.feature_metrics import kid_score, prdc
    F = a.dims
    res = {"workload": "prdc(nearest_k=5) and kid_score(subsets=100, subset_size=1000) on synthetic fp32 features", "F": F,
           "fp64_matrix_peak_tflops": FP64_MATRIX_PEAK_TF, "iters": a.iters}
    for n in a.sizes:
        real, fake = synthetic(n, F, 1, 0.0), synthetic(n, F, 2, 0.02)
        out = {}
        ms = timed_ms(lambda: out.update(prdc=prdc(real, fake, nearest_k=5)), a.iters)
        tf = 2.0 * F * 4.0 * n * n / (ms * 1e-3) / 1e12
        entry = {"prdc_ms": ms, "prdc_fp64_tflops": tf, "prdc_frac_of_peak": tf / FP64_MATRIX_PEAK_TF, "prdc": out["prdc"]}
        m = min(1000, n)
        ms = timed_ms(lambda: out.update(kid=kid_score(fake, real, subsets=100, subset_size=m)), a.iters)
        tf = 2.0 * F * 100 * 3.0 * m * m / (ms * 1e-3) / 1e12
        entry.update({"kid_ms": ms, "kid_fp64_tflops": tf, "kid_frac_of_peak": tf / FP64_MATRIX_PEAK_TF, "kid": out["kid"]})
        res[f"n{n}"] = entry
        del real, fake
    print(json.dumps(res))


if __name__ == "__main__":
    main()
