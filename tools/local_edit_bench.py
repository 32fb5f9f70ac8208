"""What a local edit costs, on one GPU in one process: Euler solves of ``--steps`` steps, timed whole.

    local    cnf.decode_local(z, ..., mask=m): the paired solve over 2B rows with a fixed mask (one uspace_pair_blend per evaluation)
    plain2B  cnf.decode on 2B rows: the same network work without the blend
    plainB   cnf.decode on B rows: what the edit alone costs today
    words    (text-to-image) decode_local with an AttentionWordMask from t = 0: every evaluation also produces its attention maps
             (uspace_uvit_forward_maps), makes the mask (uspace_mask_from_maps) and unites the two branches' masks

    python tools/local_edit_bench.py [--out profiles/local_edit.md] [--steps 20] [--rounds 5] [--only L:8,S:16]

U-ViT-L (unconditional, 32 x 32 latents, a tail write on the edited branch) and U-ViT-S-deep16 T2I (a replaced prompt).  A sample is the
host time of one solve between two device synchronisations over its number of evaluations; the arms alternate within a round; the table
gives the median and the min-max spread in ms per evaluation.  There is no threshold: the tool records."""
import argparse
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

COMMON = dict(img_size=32, patch_size=2, in_chans=4, mlp_ratio=4, qkv_bias=False, mlp_time_embed=False)
SHAPES = {"L": ("U-ViT-L", False, dict(embed_dim=1024, depth=20, num_heads=16, num_classes=-1), (8, 32)),
          "S": ("U-ViT-S-deep16 T2I", True, dict(embed_dim=512, depth=16, num_heads=8, clip_dim=768, num_clip_token=77), (4, 16))}


def arms_for(cnf, t2i, B, dev, steps, root):
    from uspace_amd.tools.local_edit import AttentionWordMask
    g = torch.Generator().manual_seed(B)
    z = torch.randn(B, 4, 32, 32, generator=g).to(dev)
    z2 = torch.cat([z, z])
    mask = torch.zeros(B, 32, 32, device=dev)
    mask[:, :, 16:] = 1.0
    sk = dict(solver="fixed", solver_fix="euler", solver_fix_step=1.0 / steps)
    if not t2i:
        kw = dict(edit_loc="tail", dissect_task="uspace_uvit", dissect_name="write_attr", t_edit=1.0, write_path_root=root, ith_attr=0,
                  write_scale=1.0, solver_kwargs=sk)
        rows = np.concatenate([np.zeros(B, np.float32), np.ones(B, np.float32)])
        return dict(local=lambda: cnf.decode_local(z, None, mask=mask, **kw)[0],
                    plain2B=lambda: cnf.decode(z2, None, **dict(kw, write_scale=rows)),
                    plainB=lambda: cnf.decode(z, None, **kw))
    ctx = torch.randn(B, 77, 768, generator=g).to(dev)
    src = torch.randn(B, 77, 768, generator=g).to(dev)
    ctx2 = torch.cat([src, ctx])
    kw = dict(dissect_name="none", solver_kwargs=sk)
    words = AttentionWordMask(token_ids=(np.array([2, 3]), np.array([2])), from_t=0.0)
    return dict(local=lambda: cnf.decode_local(z, context=ctx, mask=mask, source=dict(context=src), **kw)[0],
                plain2B=lambda: cnf.decode(z2, context=ctx2, **kw),
                plainB=lambda: cnf.decode(z, context=ctx, **kw),
                words=lambda: cnf.decode_local(z, context=ctx, mask=words, source=dict(context=src), **kw)[0])


def sample(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "local_edit.md"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default="", help="comma list of SHAPE:B, e.g. L:8,S:16")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("local_edit_bench.py measures on a ROCm device; none is visible")
    from uspace_amd import flow_matching, flow_matching_t2i
    from uspace_amd.tools.utils_uvit import get_nnet
    dev = torch.device("cuda:0")
    only = {tuple(s.split(":")) for s in a.only.split(",") if s}
    rows = []
    with tempfile.TemporaryDirectory() as root:
        table = (0.1 * np.random.default_rng(0).standard_normal((1, 4, 32, 32))).astype(np.float32)
        for k in range(1, 101):
            np.save(os.path.join(root, f"delta_{k / 100:.2f}.npy"), table)
        for key, (title, t2i, shape, batches) in SHAPES.items():
            torch.manual_seed(1234)
            net = get_nnet("uvit_t2i" if t2i else "uvit", **COMMON, **shape).to(dev).eval()
            net.use_graph = False
            cnf = (flow_matching_t2i if t2i else flow_matching).CNF(net)
            for B in batches:
                if only and (key, str(B)) not in only:
                    continue
                fns = arms_for(cnf, t2i, B, dev, a.steps, root)
                names = tuple(fns)
                with torch.no_grad():
                    for k in names:                                                      # first use (packing, workspaces) and a warm-up
                        fns[k]()
                        sample(fns[k], a.steps)
                    ms = {k: [] for k in names}
                    for r in range(a.rounds):
                        order = names[r % len(names):] + names[:r % len(names)]          # alternate, rotating who goes first
                        for k in order:
                            ms[k].append(sample(fns[k], a.steps))
                rows.append((title, B, ms))
                print(f"{title} B={B}: " + ", ".join(f"{k} {statistics.median(ms[k]):.3f} ms" for k in names), flush=True)
            del net, cnf
            torch.cuda.empty_cache()

    med = statistics.median
    fmt = lambda v: f"{med(v):.3f} ({min(v):.3f} - {max(v):.3f})" if v else "-"
    lines = ["# Local edits: the paired solve against plain decodes, and the cost of per-evaluation maps", "",
             f"`python tools/local_edit_bench.py --steps {a.steps} --rounds {a.rounds}` on {torch.cuda.get_device_name(0)}, one process, eager "
             f"(no hipGraph), Euler with {a.steps} steps, 32 x 32 latents, a half-plane mask.  A sample is the host time of one solve between "
             f"two device synchronisations over its {a.steps} evaluations; {a.rounds} samples per arm, the arms alternating; median (min - max) "
             "in ms per evaluation.", "",
             "* **local**: `decode_local` with a fixed mask: one network call over 2B rows and one `uspace_pair_blend` per evaluation.",
             "* **plain 2B** / **plain B**: `decode` on 2B / B rows with the same edit keywords.",
             "* **words**: `decode_local` with an `AttentionWordMask` from t = 0: `uspace_uvit_forward_maps`, `uspace_mask_from_maps` and the "
             "union at every evaluation.", "",
             "| network | B | local | plain 2B | plain B | words | local / plain 2B | local / plain B | words / local |",
             "|---|---|---|---|---|---|---|---|---|"]
    for title, B, ms in rows:
        w = ms.get("words", [])
        lines.append(f"| {title} | {B} | {fmt(ms['local'])} | {fmt(ms['plain2B'])} | {fmt(ms['plainB'])} | {fmt(w)} | "
                     f"{med(ms['local']) / med(ms['plain2B']):.3f} | {med(ms['local']) / med(ms['plainB']):.3f} | "
                     + (f"{med(w) / med(ms['local']):.3f}" if w else "-") + " |")
    lines += ["", "These numbers were read once and compared with no other design (a state-level blend, a fused blend in the output head, "
              "maps from a subset of the blocks): they say what the feature costs as built, not that it could not cost less.", ""]
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
