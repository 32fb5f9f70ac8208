"""Throughput of the attribute classifier and of the attribute-effect metric on the HIP kernels, images in [0, 1], seeded weights:
  images per second of ``AttributeClassifier.logits`` (quantise, normalise, tower, fc) for ResNet-50 and ResNet-18 at 224^2 and
  256^2, B = 64;
  pairs per second of ``attribute_effect`` (both members through ResNet-50 at 224^2, then the fp64 effect kernel), and of the
  effect kernel alone on 65 536 pairs of logits;
  for context only: the same module's own torch layers run eagerly by PyTorch-ROCm in fp32 on the same images,
each timed with a host clock around calls that end in a device synchronise, after a warm-up, median of the rounds.  Every arm runs
in a child process of its own under ``timeout``; the first arm that fails ends the run.  Prints one JSON line.
    python tools/attr_bench.py [--batch 64] [--rounds 5] [--arm-timeout 240]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ARMS = ("resnet50", "resnet18", "effect")


def _time(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _median_rate(n, fn, rounds):
    fn()
    fn()                                        # warm-up: weights packed, workspaces allocated, clocks up
    return n / statistics.median(_time(fn) for _ in range(rounds))


def eager_logits(m, images):
    """The module's own torch layers run by PyTorch (fp32): what the kernels replace; for context, not a path of the package."""
    import torch
    x = (images - torch.tensor(m.mean, device=images.device).view(1, 3, 1, 1)) / torch.tensor(m.std, device=images.device).view(1, 3, 1, 1)
    x = m.maxpool(torch.relu(m.bn1(m.conv1(x))))
    for layer in (m.layer1, m.layer2, m.layer3, m.layer4):
        for b in layer:
            y = torch.relu(b.bn1(b.conv1(x)))
            if m.block == "bottleneck":
                y = b.bn3(b.conv3(torch.relu(b.bn2(b.conv2(y)))))
            else:
                y = b.bn2(b.conv2(y))
            x = torch.relu(y + (x if b.downsample is None else b.downsample(x)))
    return m.fc(m.avgpool(x).flatten(1))


def run_arm(arm, B, rounds):
    import torch
    assert torch.cuda.is_available(), "attr_bench needs a ROCm device"
    from uspace_amd.libs import resnet
    from uspace_amd.tools.attr_metrics import AttributeClassifier, attribute_effect, effect_columns
    g = torch.Generator().manual_seed(1)
    out = {}
    if arm in ("resnet50", "resnet18"):
        tower = resnet.ResNet(**getattr(resnet, arm.upper()), seed=0).cuda()
        clf = AttributeClassifier(tower)
        for size in (224, 256):
            x = torch.rand(B, 3, size, size, generator=g).cuda()
            out[f"{arm}_{size}_images_per_s"] = _median_rate(B, lambda: clf.logits(x), rounds)
            with torch.no_grad():
                out[f"{arm}_{size}_torch_eager_fp32_images_per_s"] = _median_rate(B, lambda: eager_logits(tower, x), rounds)
                z, ze = clf.logits(x, quantize=False), eager_logits(tower, x)
            out[f"{arm}_{size}_rel_l2_to_torch_eager"] = float((z - ze).norm() / ze.norm())
    else:
        tower = resnet.ResNet(**resnet.RESNET50, seed=0).cuda()
        clf = AttributeClassifier(tower)
        x = torch.rand(B, 3, 224, 224, generator=g).cuda()
        y = (x + 0.1 * (2 * torch.rand(B, 3, 224, 224, generator=g).cuda() - 1)).clamp(0, 1)
        out["attribute_effect_resnet50_224_pairs_per_s"] = _median_rate(B, lambda: attribute_effect(clf, x, y, "Smiling", +1), rounds)
        n = 65536
        za, zb = torch.randn(n, 40, generator=g).cuda(), torch.randn(n, 40, generator=g).cuda()
        tgt, sg, sigma = torch.full((n,), 31, dtype=torch.int32).cuda(), torch.ones(n).cuda(), torch.ones(40).cuda()
        out["effect_kernel_pairs_per_s"] = _median_rate(n, lambda: effect_columns(za, zb, tgt, sg, sigma), rounds)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--arm-timeout", type=int, default=240)
    ap.add_argument("--arm", choices=ARMS, help="run one arm in this process (what the driver starts)")
    a = ap.parse_args()
    if a.arm:
        print("ATTR_BENCH_ARM " + json.dumps(run_arm(a.arm, a.batch, a.rounds)))
        return 0
    result = {"batch": a.batch, "rounds": a.rounds}
    for arm in ARMS:
        cmd = ["timeout", "-k", "10", str(a.arm_timeout), sys.executable, os.path.abspath(__file__), "--arm", arm, "--batch", str(a.batch),
               "--rounds", str(a.rounds)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        lines = [l for l in p.stdout.splitlines() if l.startswith("ATTR_BENCH_ARM ")]
        if p.returncode != 0 or not lines:      # nothing more is started on the device after an arm that failed
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            result["failed_arm"] = {"arm": arm, "exit_status": p.returncode}
            print(json.dumps(result))
            return 1
        result.update(json.loads(lines[-1][len("ATTR_BENCH_ARM "):]))
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
