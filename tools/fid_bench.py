"""Throughput of the FID path on the HIP kernels: Inception-v3 features (256^2 images resized to 299^2, 11.42 GFLOP per
image) at batch 50 and 200, the fp64 statistics accumulation per batch, the host sqrtm of the Frechet distance, and the same
network as torch fp32 F.conv2d on the GPU as a baseline.  Seeded weights; prints one JSON line.
    python tools/fid_bench.py [--iters 5]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

FP32_MFMA_PEAK_TF = 155.0


def torch_features(sd, x):
    """The FID network as torch fp32 ops on the GPU (BN folded), NCHW: the baseline."""
    from uspace_amd.tools.inception import ARCH
    p = {}
    for name, _ci, _co, _k, s, pad in ARCH:
        w = sd[f"{name}.conv.weight"]
        sc = sd[f"{name}.bn.weight"] / torch.sqrt(sd[f"{name}.bn.running_var"] + 1e-3)
        p[name] = (w * sc[:, None, None, None], sd[f"{name}.bn.bias"] - sd[f"{name}.bn.running_mean"] * sc, s, pad)

    def c(name, t):
        w, b, s, pad = p[name]
        return torch.relu(F.conv2d(t, w, b, stride=s, padding=pad))

    x = 2 * F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False) - 1
    x = F.max_pool2d(c("Conv2d_2b_3x3", c("Conv2d_2a_3x3", c("Conv2d_1a_3x3", x))), 3, 2)
    x = F.max_pool2d(c("Conv2d_4a_3x3", c("Conv2d_3b_1x1", x)), 3, 2)
    avg = lambda t: F.avg_pool2d(t, 3, 1, 1, count_include_pad=False)
    for n in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
        x = torch.cat([c(f"{n}.branch1x1", x), c(f"{n}.branch5x5_2", c(f"{n}.branch5x5_1", x)),
                       c(f"{n}.branch3x3dbl_3", c(f"{n}.branch3x3dbl_2", c(f"{n}.branch3x3dbl_1", x))),
                       c(f"{n}.branch_pool", avg(x))], 1)
    n = "Mixed_6a"
    x = torch.cat([c(f"{n}.branch3x3", x), c(f"{n}.branch3x3dbl_3", c(f"{n}.branch3x3dbl_2", c(f"{n}.branch3x3dbl_1", x))),
                   F.max_pool2d(x, 3, 2)], 1)
    for n in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
        b7 = c(f"{n}.branch7x7_3", c(f"{n}.branch7x7_2", c(f"{n}.branch7x7_1", x)))
        d = x
        for i in range(1, 6):
            d = c(f"{n}.branch7x7dbl_{i}", d)
        x = torch.cat([c(f"{n}.branch1x1", x), b7, d, c(f"{n}.branch_pool", avg(x))], 1)
    n = "Mixed_7a"
    d = x
    for i in range(1, 5):
        d = c(f"{n}.branch7x7x3_{i}", d)
    x = torch.cat([c(f"{n}.branch3x3_2", c(f"{n}.branch3x3_1", x)), d, F.max_pool2d(x, 3, 2)], 1)
    for n, mx in (("Mixed_7b", False), ("Mixed_7c", True)):
        t = c(f"{n}.branch3x3_1", x)
        u = c(f"{n}.branch3x3dbl_2", c(f"{n}.branch3x3dbl_1", x))
        pool = F.max_pool2d(x, 3, 1, 1) if mx else avg(x)
        x = torch.cat([c(f"{n}.branch1x1", x), c(f"{n}.branch3x3_2a", t), c(f"{n}.branch3x3_2b", t),
                       c(f"{n}.branch3x3dbl_3a", u), c(f"{n}.branch3x3dbl_3b", u), c(f"{n}.branch_pool", pool)], 1)
    return x.mean((2, 3))


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "fid_bench needs a ROCm device"
    from uspace_amd.tools.fid_score import FIDStatistics, calculate_frechet_distance
    from uspace_amd.tools.inception import GFLOP_PER_IMAGE, InceptionV3
    model = InceptionV3(seed=0).cuda()
    res = {"workload": "FID Inception-v3 features, 256^2 -> 299^2, fp32 MFMA", "gflop_per_img": GFLOP_PER_IMAGE,
           "fp32_mfma_peak_tflops": FP32_MFMA_PEAK_TF}
    g = torch.Generator().manual_seed(1)
    for B in (50, 200):
        x = torch.rand(B, 3, 256, 256, generator=g).cuda()
        dt = timed(lambda: model.features(x, chunk=B), a.iters)
        tf = GFLOP_PER_IMAGE * B / dt / 1e3
        res[f"b{B}"] = {"ms_per_batch": dt * 1e3, "img_per_s": B / dt, "tflops": tf, "frac_of_peak": tf / FP32_MFMA_PEAK_TF}
    feat = model.features(x)
    st = FIDStatistics(2048, device="cuda", model=model)
    st.update_features(feat)
    res["stats_ms_per_batch200"] = timed(lambda: st.update_features(feat), a.iters) * 1e3
    mu, sigma = st.mu, st.sigma
    t0 = time.perf_counter()
    calculate_frechet_distance(mu, sigma, mu + 0.01, sigma + 0.01 * np.eye(2048))
    res["host_sqrtm_s"] = time.perf_counter() - t0
    sd = {k: v.detach().float() for k, v in model.state_dict().items()}
    with torch.no_grad():
        base = torch_features(sd, x)
        res["torch_fp32_rel_diff"] = float((base - feat).norm() / feat.norm())
        dt = timed(lambda: torch_features(sd, x), max(1, a.iters // 2))
    res["torch_fp32_b200"] = {"ms_per_batch": dt * 1e3, "img_per_s": 200 / dt, "tflops": GFLOP_PER_IMAGE * 200 / dt / 1e3}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
