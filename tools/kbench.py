#!/usr/bin/env python3
"""Kernel micro-benchmarks at the BASELINE shapes (run on the GPU box): GEMMs, attention, LayerNorm.
``--long``: the two streaming attention kernels alone, long and wide (profiles/attention_long.md, profiles/attention_stream.md)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from uspace_amd import _hip  # noqa: E402


def timeit(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e-3


BF16_NOMINAL = 2.5e15       # dense bf16 MFMA rate of the MI355X, FLOP/s


MIN_WINDOW = 0.1            # seconds a row of --long is timed over, at the least


def timeit_window(fn):
    """timeit over as many launches as fill MIN_WINDOW (a pilot of 50 gives the count; 1.2 x so that a faster second pass still fills it)."""
    t = timeit(fn, reps=50, warm=5)
    return timeit(fn, reps=max(50, int(1.2 * MIN_WINDOW / t) + 1), warm=0)


def attention_long_rows():
    """The streaming attention kernels.  The long form (attention_long.hip, uspace_attention_long_bf16) at 64 x 64 latents -- L = 1 025
    (unconditional) and 1 102 (T2I) at B * H = 16 and 1 024 -- and at L = 334 beside the resident kernel: time, TFLOP/s (4 L^2 64 per
    head) and the share of the nominal rate.  The wide form (attention_wide.hip, uspace_attention_wide_bf16) at C = 512, N = 4 096 and B = 1, 2, 8: the
    plan's 1-, 2- and 4-wave branches, 4 N^2 C per image."""
    H = 16
    print("| kernel | B x H | L | key_scale | us | TFLOP/s | of 2.5 PF |\n|---|---|---|---|---|---|---|")
    for L in (1025, 1102, 334):
        for B in (1, 64):
            qkv = torch.randn(B * L, 3 * H * 64, device="cuda").to(torch.bfloat16)
            for scaled in (False, True):
                ks = torch.exp(torch.rand(B, L, device="cuda") * 2 - 1) if scaled else None
                forms = [("long", _hip.attention_long)] + ([("resident", _hip.attention)] if L <= 336 else [])
                for name, fn in forms:
                    t = timeit_window(lambda: fn(qkv, B, L, H, key_scale=ks))
                    fl = 4.0 * L * L * 64 * B * H
                    print(f"| {name} | {B} x {H} | {L} | {'yes' if scaled else 'no'} | {t * 1e6:.1f} | {fl / t / 1e12:.1f} | {fl / t / BF16_NOMINAL:.3f} |")
    N, C = 4096, 512
    for B in (1, 2, 8):
        q, k, v = (torch.randn(B * N, C, device="cuda").to(torch.bfloat16) for _ in range(3))
        t = timeit_window(lambda: _hip.attention_wide(q, k, v, B, N, C, C ** -0.5))
        fl = 4.0 * N * N * C * B
        print(f"| wide C={C} | {B} x 1 | {N} | no | {t * 1e6:.1f} | {fl / t / 1e12:.1f} | {fl / t / BF16_NOMINAL:.3f} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--long", action="store_true", help="only the long-sequence attention rows")
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--L", type=int, default=257)
    ap.add_argument("--D", type=int, default=1024)
    a = ap.parse_args()
    if a.long:
        return attention_long_rows()
    M, D = a.B * a.L, a.D
    dev = "cuda"
    bf = torch.bfloat16
    x = torch.randn(M, D, device=dev).to(bf)
    x2 = torch.randn(M, D, device=dev).to(bf)
    f = torch.randn(M, 4 * D, device=dev).to(bf)
    res = torch.randn(M, D, device=dev)
    shapes = [("qkv", D, 3 * D), ("proj", D, D), ("fc1", D, 4 * D), ("fc2", 4 * D, D), ("skip", 2 * D, D)]
    tot_t, tot_f = 0.0, 0.0
    for name, K, N in shapes:
        W = (torch.randn(N, K, device=dev) * 0.02).to(bf)
        b = torch.zeros(N, device=dev)
        if name == "qkv":
            o = torch.empty(M, N, device=dev, dtype=bf)
            fn = lambda: _hip.gemm(x, W, out_bf16=o)
        elif name == "fc1":
            o = torch.empty(M, N, device=dev, dtype=bf)
            fn = lambda: _hip.gemm(x, W, bias=b, gelu=True, out_bf16=o)
        elif name == "fc2":
            o = torch.empty(M, N, device=dev, dtype=bf)
            fn = lambda: _hip.gemm(f, W, bias=b, resid=res, out_f32=res, out_bf16=o)
        elif name == "proj":
            fn = lambda: _hip.gemm(x, W, bias=b, resid=res, out_f32=res)
        else:
            fn = lambda: _hip.gemm(x, W, A2=x2, bias=b, out_f32=res)
        t = timeit(fn)
        fl = 2.0 * M * N * K
        cnt = {"qkv": 21, "proj": 21, "fc1": 21, "fc2": 21, "skip": 10}[name]
        tot_t += t * cnt
        tot_f += fl * cnt
        print(f"gemm {name:5s} M={M} N={N} K={K}: {t*1e6:9.1f} us  {fl/t/1e12:7.1f} TFLOP/s")
    print(f"  -> all GEMMs of one forward: {tot_t*1e3:.2f} ms, {tot_f/tot_t/1e12:.1f} TFLOP/s aggregate")
    # ablation: the fc1 shape without the GELU in its epilogue (bias + bf16 store only)
    W = (torch.randn(4 * D, D, device=dev) * 0.02).to(bf)
    b = torch.zeros(4 * D, device=dev)
    o = torch.empty(M, 4 * D, device=dev, dtype=bf)
    t = timeit(lambda: _hip.gemm(x, W, bias=b, out_bf16=o))
    print(f"gemm fc1 without GELU (ablation):        {t*1e6:9.1f} us  {2.0*M*4*D*D/t/1e12:7.1f} TFLOP/s")
    H = D // 64
    qkv = torch.randn(M, 3 * D, device=dev).to(bf)
    t = timeit(lambda: _hip.attention(qkv, a.B, a.L, H))
    fl = 4.0 * a.L * a.L * D * a.B
    byts = M * 3 * D * 2 + M * D * 2
    print(f"attention B={a.B} L={a.L} H={H}: {t*1e6:9.1f} us  {fl/t/1e12:7.1f} TFLOP/s  {byts/t/1e9:7.0f} GB/s")
    xs = torch.randn(M, D, device=dev)
    g, bb = torch.ones(D, device=dev), torch.zeros(D, device=dev)
    t = timeit(lambda: _hip.layernorm(xs, g, bb))
    print(f"layernorm M={M} D={D}: {t*1e6:9.1f} us  {M*D*6/t/1e9:7.0f} GB/s (algorithmic 6 B/elem)")


if __name__ == "__main__":
    main()
