"""Throughput of the DINO towers and of the structure distance on the HIP kernels, 256^2 images in [0, 1], seeded weights:
  images per second of preprocess + tower (``pooler_output``) at DINOv2 ViT-L/14 and at DINO ViT-B/8, both at 224^2, and pairs per
  second of ``structure_distance`` (ViT-B/8, last-layer keys of both members, then the self-similarity kernel) and of that kernel alone,
each timed with a host clock around calls that end in a device synchronise, after a warm-up, median of the rounds.  Prints one
JSON line.
    python tools/dino_bench.py [--batch 64] [--rounds 5]"""
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
    assert torch.cuda.is_available(), "dino_bench needs a ROCm device"
    from uspace_amd.libs.dino import DINO_B8, DINOV2_L14, DinoVisionTransformer
    from uspace_amd.tools.dino_metrics import DinoFeatures, self_similarity_mse, structure_distance
    B, R = a.batch, a.size
    g = torch.Generator().manual_seed(1)
    x = torch.rand(B, 3, R, R, generator=g).cuda()
    y = (x + 0.1 * (2 * torch.rand(B, 3, R, R, generator=g).cuda() - 1)).clamp(0, 1)
    vitl = DinoVisionTransformer(seed=0, **DINOV2_L14).cuda()
    vitb8 = DinoVisionTransformer(seed=0, **DINO_B8).cuda()
    fl, fb = DinoFeatures(vitl, B), DinoFeatures(vitb8, B)
    keys = vitb8.keys(vitb8.preprocess(torch.cat([x[:32], y[:32]])))
    ka, kb = keys[:32], keys[32:]
    chunk = 32
    arms = {
        "dinov2_vitl14_features": (B, lambda: fl.features(x)),
        "dino_vitb8_features": (B, lambda: fb.features(x)),
        "structure_distance_vitb8": (B, lambda: structure_distance(vitb8, x, y, chunk=chunk)),
        "self_similarity_kernel_785x768": (32, lambda: self_similarity_mse(ka, kb)),
    }
    for _n, fn in arms.values():                # warm-up: weights packed, workspaces allocated, clocks up
        fn()
        fn()
    times = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, (_n, fn) in arms.items():
            times[k].append(_time(fn))
    res = {"workload": f"DINO towers at 224^2 from {R}^2 images, bf16 MFMA; structure distance on 785 x 768 keys", "device": torch.cuda.get_device_name(0),
           "batch": B, "rounds": a.rounds, "structure_chunk_pairs": chunk}
    for k, ts in times.items():
        n = arms[k][0]
        res[k] = {"per_s_median": n / statistics.median(ts), "per_s_best": n / min(ts), "ms_per_call_median": statistics.median(ts) * 1e3,
                  "items_per_call": n}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
