"""Throughput of the ArcFace identity tower and of the ID similarity on the HIP kernels, 256^2 images in [0, 1], seeded weights:
  images per second of preprocess (pool, crop, pool to 112^2) + IR-SE50;
  pairs per second of ``IDSimilarity`` (both members through the tower, then the fp64 dot product);
  pairs per second of a whole ``PairMetrics.update`` with ``identity=`` (LPIPS-alex, SSIM, PSNR and the ID similarity),
each timed with a host clock around calls that end in a device synchronise, after a warm-up, median of the rounds.  Prints one
JSON line.
    python tools/id_bench.py [--batch 64] [--rounds 5]"""
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
    assert torch.cuda.is_available(), "id_bench needs a ROCm device"
    from uspace_amd.libs.arcface import IR_SE50, Backbone
    from uspace_amd.tools.id_metrics import IDSimilarity
    from uspace_amd.tools.lpips import LPIPS
    from uspace_amd.tools.pair_metrics import PairMetrics
    B, R = a.batch, a.size
    g = torch.Generator().manual_seed(1)
    x = torch.rand(B, 3, R, R, generator=g).cuda()
    y = (x + 0.1 * (2 * torch.rand(B, 3, R, R, generator=g).cuda() - 1)).clamp(0, 1)
    tower = Backbone(seed=0, **IR_SE50).cuda()
    metric = IDSimilarity(tower)
    pm = PairMetrics(device="cuda", lpips=LPIPS("alex", seed=0).cuda(), identity=tower)

    def update():
        pm.reset()
        pm.update(x, y)

    arms = {
        "ir_se50_features": (B, lambda: metric.features(x)),
        "id_similarity": (B, lambda: metric(x, y)),
        "pair_metrics_update_with_identity": (B, update),
    }
    for _n, fn in arms.values():                # warm-up: weights packed, workspaces allocated, clocks up
        fn()
        fn()
    times = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, (_n, fn) in arms.items():
            times[k].append(_time(fn))
    res = {"workload": f"ArcFace IR-SE50 at 112^2 from {R}^2 images, fp32 MFMA; ID similarity; PairMetrics with identity=",
           "device": torch.cuda.get_device_name(0), "batch": B, "rounds": a.rounds, "tower_chunk_images": metric.chunk}
    for k, ts in times.items():
        n = arms[k][0]
        res[k] = {"per_s_median": n / statistics.median(ts), "per_s_best": n / min(ts), "ms_per_call_median": statistics.median(ts) * 1e3,
                  "items_per_call": n}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
