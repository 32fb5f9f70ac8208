"""Throughput of the SegFormer tower and of the segmentation-consistency metric on the HIP kernels, images in [0, 1], seeded weights:
  label maps per second of ``SegFormer.labels`` (normalise, tower, fused resize + argmax) for MiT-B5 at 512^2 (B = 8) and MiT-B2 at
  256^2 (B = 32), 19 labels;
  pairs per second of ``segmentation_consistency`` (both members through MiT-B2 at 256^2, then the two pair reductions), and of the
  reductions alone on 64 pairs of 512^2 label maps;
  per-stage times of one MiT-B5 forward at 512^2 from the launch recorder (GEMMs by shape; the attention_kv launches are not
  recorded), and the wall time of the head (tap of the last encoder stage against the whole forward),
each timed with a host clock around calls that end in a device synchronise, after a warm-up, median of the rounds.  Every arm runs
in a child process of its own under ``timeout``; the first arm that fails ends the run.  Prints one JSON line.  Read once: no
number here is compared against another design.
    python tools/seg_bench.py [--rounds 5] [--arm-timeout 240]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ARMS = ("b5_512", "b2_256", "metric")


def _time(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _median_time(fn, rounds):
    fn()
    fn()                                        # warm-up: weights packed, workspaces allocated, clocks up
    return statistics.median(_time(fn) for _ in range(rounds))


def run_arm(arm, rounds):
    import torch
    assert torch.cuda.is_available(), "seg_bench needs a ROCm device"
    from uspace_amd import _hip
    from uspace_amd.libs import segformer
    from uspace_amd.tools.seg_metrics import label_overlap, region_difference, segmentation_consistency
    g = torch.Generator().manual_seed(1)
    out = {}
    if arm in ("b5_512", "b2_256"):
        preset, size, B = (segformer.MIT_B5, 512, 8) if arm == "b5_512" else (segformer.MIT_B2, 256, 32)
        tower = segformer.SegFormer(**preset, num_labels=19, seed=0).cuda()
        x = torch.rand(B, 3, size, size, generator=g).cuda()
        out[f"{arm}_labels_per_s"] = B / _median_time(lambda: tower.labels(x), rounds)
        out[f"{arm}_logits_per_s"] = B / _median_time(lambda: tower.logits_nhwc(x), rounds)
        n_enc = len(tower.stage_shapes(size, size)) - 4
        t_enc = _median_time(lambda: tower.tap(x, n_enc), rounds)
        t_all = _median_time(lambda: tower.tap(x, n_enc + 3), rounds)
        out[f"{arm}_encoder_ms_per_image"], out[f"{arm}_head_ms_per_image"] = 1e3 * t_enc / B, 1e3 * (t_all - t_enc) / B
        if arm == "b5_512":
            _hip.prof_all_begin()
            tower.logits_nhwc(x[:1])
            recs = _hip.prof_all_end()
            out["b5_512_one_image_gemm_ms_by_shape"] = sorted(
                ([r["M"], r["N"], r["K"], r["launches"], round(r["total_ms"], 3)] for r in recs if r["kind"] == 0), key=lambda r: -r[4])[:12]
            out["b5_512_one_image_gemm_ms"] = sum(r["total_ms"] for r in recs if r["kind"] == 0)
            out["recorder_dropped"] = _hip.prof_dropped()
    else:
        tower = segformer.SegFormer(**segformer.MIT_B2, num_labels=19, seed=0).cuda()
        B = 32
        x = torch.rand(B, 3, 256, 256, generator=g).cuda()
        y = (x + 0.1 * (2 * torch.rand(B, 3, 256, 256, generator=g).cuda() - 1)).clamp(0, 1)
        out["segmentation_consistency_b2_256_pairs_per_s"] = B / _median_time(lambda: segmentation_consistency(tower, x, y, region=[1, 2]), rounds)
        n = 64
        la = torch.randint(0, 19, (n, 64, 64), generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2).to(torch.uint8).cuda().contiguous()
        lb = la.roll(3, 2).contiguous()
        a, b = torch.rand(n, 3, 512, 512, generator=g).cuda(), torch.rand(n, 3, 512, 512, generator=g).cuda()
        out["pair_counts_512_pairs_per_s"] = n / _median_time(lambda: label_overlap(la, lb, 19), rounds)
        out["region_sse_512_pairs_per_s"] = n / _median_time(lambda: region_difference(a, b, la, lb, [1, 2], 19), rounds)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--arm-timeout", type=int, default=240)
    ap.add_argument("--arm", choices=ARMS, help="run one arm in this process (what the driver starts)")
    a = ap.parse_args()
    if a.arm:
        print("SEG_BENCH_ARM " + json.dumps(run_arm(a.arm, a.rounds)))
        return 0
    result = {"rounds": a.rounds}
    for arm in ARMS:
        cmd = ["timeout", "-k", "10", str(a.arm_timeout), sys.executable, os.path.abspath(__file__), "--arm", arm, "--rounds", str(a.rounds)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        lines = [l for l in p.stdout.splitlines() if l.startswith("SEG_BENCH_ARM ")]
        if p.returncode != 0 or not lines:      # nothing more is started on the device after an arm that failed
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            result["failed_arm"] = {"arm": arm, "exit_status": p.returncode}
            print(json.dumps(result))
            return 1
        result.update(json.loads(lines[-1][len("SEG_BENCH_ARM "):]))
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
