"""Throughput of the CLIP-score path on the HIP kernels at the CLIP-L shape (ViT-L/14 at 224^2: 257 tokens, width 1024, 24 layers;
text tower 77 x 768, 12 layers) with seeded weights: images/s of ``preprocess + vision forward`` from 256^2 samples and of a whole
``CLIPScore.update`` (both towers, projections, cosine; tokenisation by a stub), at batch 16 and 64.  Timed with HIP events on
the launching stream after a warm-up of every shape; the median and the spread of ``--reps`` windows of ``--iters`` calls each.
Prints one JSON line.
    python tools/clip_score_bench.py [--iters 5] [--reps 5]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


class WordTokenizer:
    """Stands in for the HF tokenizer (its files are not needed for a timing): BOS, one id per word, EOS padding to 77."""

    def __call__(self, text, truncation=True, max_length=77, padding="max_length", return_tensors="pt", **_kw):
        rows = []
        for t in text:
            ids = [49406] + [sum((i + 1) * ord(ch) for i, ch in enumerate(w)) % 49000 for w in t.split()][:max_length - 2]
            rows.append(ids + [49407] * (max_length - len(ids)))
        return {"input_ids": torch.tensor(rows, dtype=torch.long)}


def vision_gflop_per_image(c):
    """GEMM and attention operations of one image through the tower (2 x multiply-adds), from the shapes."""
    T = (c["image_size"] // c["patch_size"]) ** 2 + 1
    D, Fd = c["hidden_size"], c["intermediate_size"]
    per_layer = 2 * T * (4 * D * D + 2 * D * Fd) + 4 * T * T * D
    patch = 2 * (T - 1) * D * 3 * c["patch_size"] ** 2
    return (c["num_hidden_layers"] * per_layer + patch + 2 * D * c["projection_dim"]) / 1e9


def timed_ms(fn, iters, reps):
    """ms per call: median and (min, max) over ``reps`` event-timed windows of ``iters`` calls."""
    fn()
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "clip_score_bench needs a ROCm device"
    from uspace_amd.libs.clip import CLIP_L_TEXT, CLIP_L_VISION, CLIPTextProjection, CLIPTextTransformer, CLIPVisionTransformer
    from uspace_amd.tools.clip_score import CLIPScore
    torch.manual_seed(0)
    vision, text, proj = CLIPVisionTransformer(**CLIP_L_VISION), CLIPTextTransformer(**CLIP_L_TEXT), CLIPTextProjection(768, 768)
    metric = CLIPScore(vision, text, proj, WordTokenizer(), device="cuda")
    gf = vision_gflop_per_image(CLIP_L_VISION)
    res = {"workload": "CLIP score, ViT-L/14 at 224^2 from 256^2 samples, seeded weights", "vision_gflop_per_img": gf}
    g = torch.Generator().manual_seed(1)
    for B in (16, 64):
        x = torch.rand(B, 3, 256, 256, generator=g).cuda()
        prompts = ["a photo of a small dog on a green lawn number %d" % i for i in range(B)]
        pre = timed_ms(lambda: vision.preprocess(x), a.iters, a.reps)
        vis = timed_ms(lambda: metric.image_features(x), a.iters, a.reps)
        upd = timed_ms(lambda: metric.update(x, prompts), a.iters, a.reps)
        res[f"b{B}"] = {"preprocess_ms": pre[0], "image_features_ms": vis[0], "image_features_ms_min_max": vis[1:],
                        "image_features_img_per_s": B / vis[0] * 1e3, "image_features_tflops": gf * B / vis[0],
                        "update_ms": upd[0], "update_ms_min_max": upd[1:], "update_img_per_s": B / upd[0] * 1e3}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
