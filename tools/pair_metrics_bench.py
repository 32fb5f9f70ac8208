"""Throughput of the paired metrics on the HIP kernels, 256^2 image pairs in [0, 1], seeded LPIPS weights: pairs per second of
  LPIPS (alex), LPIPS (vgg), SSIM, PSNR and one whole PairMetrics.update (alex; quantisation, the three metrics),
each timed with a host clock around calls that end in a device synchronise, after a warm-up, median of the rounds.  Prints
one JSON line.
    python tools/pair_metrics_bench.py [--batch 64] [--rounds 5]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def _time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--size", type=int, default=256)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "pair_metrics_bench needs a ROCm device"
    from uspace_amd.tools.lpips import LPIPS
    from uspace_amd.tools.pair_metrics import PairMetrics, psnr, ssim
    B, R = a.batch, a.size
    g = torch.Generator().manual_seed(1)
    x = torch.rand(B, 3, R, R, generator=g).cuda()
    y = (x + 0.1 * (2 * torch.rand(B, 3, R, R, generator=g).cuda() - 1)).clamp(0, 1)
    alex, vgg = LPIPS("alex", seed=0).cuda(), LPIPS("vgg", seed=0).cuda()
    pm = PairMetrics(device="cuda", lpips=alex)

    def update():
        pm.reset()
        pm.update(x, y)
    arms = {
        "lpips_alex": lambda: alex(x, y, normalize=True),
        "lpips_vgg": lambda: vgg(x, y, normalize=True),
        "ssim": lambda: ssim(x, y),
        "psnr": lambda: psnr(x, y),
        "pair_metrics_update": update,
    }
    for fn in arms.values():                    # warm-up: weights packed, workspaces allocated, clocks up
        fn()
        fn()
    times = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, fn in arms.items():
            times[k].append(_time(fn))
    res = {"workload": f"paired metrics, {R}^2 image pairs, fp32 MFMA backbones, fp64 sums", "device": torch.cuda.get_device_name(0),
           "batch": B, "rounds": a.rounds, "lpips_vgg_chunk": vgg.default_chunk(B, R, R), "lpips_alex_chunk": alex.default_chunk(B, R, R)}
    for k, ts in times.items():
        res[k] = {"pairs_per_s_median": B / statistics.median(ts), "pairs_per_s_best": B / min(ts),
                  "ms_per_batch_median": statistics.median(ts) * 1e3}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
