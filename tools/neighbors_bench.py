"""Readings of the nearest-neighbour path on the HIP kernels (no gate: there is no earlier path to compare with).

``nearest_neighbors`` (``uspace_metric_topk``: norms, the fp64 Gram tiles with the top-k consumer, the refinement) on synthetic
feature banks at 50 000 x 50 000 x 2 048 with k = 1 and k = 16: wall time (HIP events, after a warm-up) and the fp64 FLOP/s of the
Gram part (2 F per pair; the insertion path and the refinement are not counted).  The same sharded (bank rows 16 384 at a time,
merged on the device), ``authenticity`` at that size (two such calls), and the refinement pass alone: the per-kernel device times of
one call from ``torch.profiler`` where it reports them, and a call against a bank of only k rows (one column tile, so nearly all of
it is the refinement of nx k pairs; its rows stay in cache, which a real bank's do not).
Yardsticks on the same box in the same run: ``uspace_metric_manifold`` at the same shape (the same engine with the cheapest
consumer, min_d2 only) and fp64 ``torch.cdist`` + ``topk`` in row chunks that fit.
Also the box's device-to-device copy bandwidth.  Prints one JSON line; the reading is kept in profiles/neighbors.md.
    python tools/neighbors_bench.py [--iters 2] [--reps 3] [--n 50000] [--dims 2048]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

FP64_MATRIX_PEAK_TF = 78.6        # MI355X data sheet, fp64 matrix


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
    """Feature-like banks: clusters in a low-dimensional subspace plus noise and a common offset (|x|^2 >> d^2)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    centers = 3.0 * torch.randn(64, 16, generator=g, device="cuda")
    lat = centers[torch.randint(0, 64, (n,), generator=g, device="cuda")] + torch.randn(n, 16, generator=g, device="cuda")
    basis = torch.randn(16, F, generator=g, device="cuda") / 4
    return (lat @ basis + 0.05 * torch.randn(n, F, generator=g, device="cuda") + 1.0 + shift).contiguous()


def torch_topk(x, y, k, chunk=4096):
    """fp64 ``torch.cdist`` (squared) + ``topk`` of row chunks against the whole bank."""
    yd = y.double()
    d2, idx = [], []
    for lo in range(0, x.shape[0], chunk):
        d = torch.cdist(x[lo:lo + chunk].double(), yd).square_()
        v, i = torch.topk(d, k, dim=1, largest=False)
        d2.append(v)
        idx.append(i)
    return torch.cat(d2), torch.cat(idx)


def kernel_times_ms(fn):
    """{kernel name: device ms} of one call, from torch.profiler; None where it does not report the library's kernels."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for e in prof.key_averages():
            t = getattr(e, "device_time_total", None)
            if t is None:
                t = getattr(e, "cuda_time_total", 0.0)
            for name in ("TopkConsumer", "topk_refine_kernel", "norms_kernel"):
                if name in e.key:
                    out[name] = out.get(name, 0.0) + t / 1e3
        return out or None
    except Exception as exc:                                   # a reading that is missing is reported as missing
        return {"error": repr(exc)[:200]}


def copy_gb_per_s():
    a = torch.empty(1 << 28, dtype=torch.float32, device="cuda")
    b = torch.empty_like(a)
    ms = timed_ms(lambda: b.copy_(a), 10, 3)[0]
    return 2.0 * a.numel() * 4 / (ms * 1e-3) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--dims", type=int, default=2048)
    ap.add_argument("--shard-rows", type=int, default=16384)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "neighbors_bench needs a ROCm device"
    from uspace_amd import _hip
    from uspace_amd.tools.neighbors import authenticity, nearest_neighbors
    n, F = a.n, a.dims
    x, y = synthetic(n, F, 1, 0.02), synthetic(n, F, 2, 0.0)
    flop = 2.0 * F * float(n) * n
    tf = lambda ms: flop / (ms * 1e-3) / 1e12
    res = {"workload": "nearest_neighbors (uspace_metric_topk) on synthetic banks; yardsticks uspace_metric_manifold and torch.cdist + topk in fp64",
           "nx": n, "ny": n, "F": F, "fp64_matrix_peak_tflops": FP64_MATRIX_PEAK_TF, "iters": a.iters, "reps": a.reps,
           "copy_gb_per_s": copy_gb_per_s()}
    ws = _hip.metric_workspace(n, n, device=x.device)
    ms = timed_ms(lambda: _hip.metric_manifold(x, y, None, want_count=False, ws=ws), a.iters, a.reps)
    res["manifold_min_d2"] = {"ms": ms[0], "ms_min_max": ms[1:], "gram_fp64_tflops": tf(ms[0]), "frac_of_peak": tf(ms[0]) / FP64_MATRIX_PEAK_TF}
    manifold_ms = ms[0]
    for k in (1, 16):
        ms = timed_ms(lambda: nearest_neighbors(x, y, k), a.iters, a.reps)
        ms_s = timed_ms(lambda: nearest_neighbors(x, y, k, shard_rows=a.shard_rows), a.iters, a.reps)
        ms_r = timed_ms(lambda: _hip.metric_topk(x, y[:k], k), a.iters, a.reps)
        ms_t = timed_ms(lambda: torch_topk(x, y, k), 1, a.reps)
        d2, idx = nearest_neighbors(x, y, k)
        d2_t, idx_t = torch_topk(x, y, k)
        res[f"topk_k{k}"] = {"ms": ms[0], "ms_min_max": ms[1:], "gram_fp64_tflops": tf(ms[0]), "frac_of_peak": tf(ms[0]) / FP64_MATRIX_PEAK_TF,
                             "over_manifold": ms[0] / manifold_ms, "sharded_ms": ms_s[0], "sharded_ms_min_max": ms_s[1:],
                             "shard_rows": a.shard_rows, "bank_of_k_rows_ms": ms_r[0], "bank_of_k_rows_ms_min_max": ms_r[1:],
                             "kernel_ms": kernel_times_ms(lambda: nearest_neighbors(x, y, k)),
                             "torch_fp64_ms": ms_t[0], "torch_fp64_ms_min_max": ms_t[1:], "torch_over_hip": ms_t[0] / ms[0],
                             "indices_equal_torch": float((idx.long() == idx_t).double().mean()),
                             "max_rel_d2_vs_torch": float(((d2 - d2_t).abs() / d2_t.clamp_min(1e-300)).max())}
        del d2, idx, d2_t, idx_t
    ms = timed_ms(lambda: authenticity(x, y), 1, a.reps)
    res["authenticity"] = {"ms": ms[0], "ms_min_max": ms[1:], "authenticity_pct": authenticity(x, y)["authenticity_pct"]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
