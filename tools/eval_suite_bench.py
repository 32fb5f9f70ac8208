"""Throughput of the one-pass evaluation path on the HIP kernels, 256^2 images (resized to 299^2), seeded weights:
  (a) features()            the pool features alone (what FID needs),
  (b) features() + tap(14)  how both feature sets were obtained before suite(): two walks of the network,
  (c) suite()               pool + spatial features from one walk,
interleaved round by round in one process on one device after a warm-up, and the time of inception_score at 50 000 x 1008
and of the logits head per batch.  Prints one JSON line.
    python tools/eval_suite_bench.py [--batch 200] [--rounds 5]"""
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
    ap.add_argument("--batch", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "eval_suite_bench needs a ROCm device"
    from uspace_amd.tools.inception import InceptionHead, InceptionV3
    from uspace_amd.tools.inception_score import inception_score
    model = InceptionV3(seed=0).cuda()
    head = InceptionHead(seed=1).cuda()
    B = a.batch
    g = torch.Generator().manual_seed(1)
    x = torch.rand(B, 3, 256, 256, generator=g).cuda()
    arms = {
        "a_features": lambda: model.features(x, chunk=B),
        "b_features_plus_tap14": lambda: (model.features(x, chunk=B), model.tap(x, 14, chunk=B)),
        "c_suite": lambda: model.suite(x, chunk=B),
    }
    for fn in arms.values():                    # warm-up: weights packed, workspace allocated, clocks up
        fn()
        fn()
    times = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, fn in arms.items():
            times[k].append(_time(fn))
    res = {"workload": "Inception-v3 evaluation features, 256^2 -> 299^2, fp32 MFMA", "device": torch.cuda.get_device_name(0),
           "batch": B, "rounds": a.rounds}
    for k, ts in times.items():
        res[k] = {"img_per_s_median": B / statistics.median(ts), "img_per_s_best": B / min(ts),
                  "ms_per_batch_median": statistics.median(ts) * 1e3}
    res["c_over_a"] = res["c_suite"]["img_per_s_median"] / res["a_features"]["img_per_s_median"]
    res["c_over_b"] = res["c_suite"]["img_per_s_median"] / res["b_features_plus_tap14"]["img_per_s_median"]
    pool = model.features(x, chunk=B)
    head.logits(pool)
    res["logits_ms_per_batch"] = statistics.median(_time(lambda: head.logits(pool)) for _ in range(a.rounds)) * 1e3
    logits = (2.5 * torch.randn(50000, 1008, generator=g)).cuda()
    inception_score(logits, 10)
    res["inception_score_50000x1008_ms"] = statistics.median(_time(lambda: inception_score(logits, 10)) for _ in range(a.rounds)) * 1e3
    res["inception_score_50000x1008_1split_ms"] = statistics.median(_time(lambda: inception_score(logits, 1))
                                                                    for _ in range(a.rounds)) * 1e3
    print(json.dumps(res))


if __name__ == "__main__":
    main()
