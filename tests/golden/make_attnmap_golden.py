#!/usr/bin/env python3
"""Generate tests/golden/attn_maps_t2i.npz by IMPORTING the reference (see make_golden.py and _refshim.py: the reference is
imported from where it lies, only data is stored).

    python tests/golden/make_attnmap_golden.py

The reference's editable attention path (libs/uvit_t2i.py:91-107) hands the [B, H, L, L] softmax of every block to
tools/utils_t2i.py:265-296 editing_attention_map_vit, which -- on decode, with ``vis_am_path`` set -- passes it to
tools/utils_t2i.py:141-193 vis_attention_map BEFORE the p2p edit (:283 precedes :286).  Here that function is replaced by a recorder
(the reference's own cannot run on the tiny network: it rearranges the image tokens to 16 x 16 and loads a tokenizer), which keeps
what the picture is made of:  attention_map.mean(1)[:, 1 + 77:, 1:1 + 77]  per block.

What is pinned, at t = 0.30 (digit "0.30", one of the nine the reference draws at):
  tiny_edit/{i}, tiny_plain/{i}   the tiny T2I network of tiny_t2i.npz (state dict, x, ctx from that file; B = 3), blocks 0 .. 2,
                                  with the p2p edit live (t_edit 0.5, multiplier 3, ids of make_golden.make_p2p_t2i, every block) and
                                  without (t_edit 0.1 < t: the edit path still runs, nothing is rescaled)
  S_edit/{i}                      the seed-regenerated U-ViT-S T2I of big_S_t.npz (x, ctx from that file; B = 2), blocks 0, 8, 16,
                                  edit live (the first two id sets)
  *_block_diff                    max |edit - plain| per block: 0 for block 0 only (the edit of block i acts on P.V, i.e. on the
                                  residual stream the LATER blocks read); recorded for the S network too, whose plain maps are not stored
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refshim  # noqa: E402
from make_golden import COMMON, SHAPES, TINY, WEIGHT_SEED, expand_t, sd_sha256  # noqa: E402

T_VIS = 0.30
N_CTX = 77
IDS = [np.array([3, 5], dtype=np.int64), np.array([], dtype=np.int64), np.array([0, 76, 76], dtype=np.int64)]
S_BLOCKS = (0, 8, 16)


def record(ut2i, m, x, ctx, t_edit):
    """The reference forward with vis_attention_map replaced by a recorder -> [per block: [B, n_img, 77] fp32], prediction."""
    maps = []

    def recorder(attention_map, timestep_digit, **kwargs):
        assert timestep_digit == f"{T_VIS:.2f}" and kwargs["_counter"]["block_id"] == len(maps)
        maps.append(attention_map.mean(1)[:, 1 + N_CTX:, 1:1 + N_CTX].clone().numpy().astype(np.float32))

    orig = ut2i.vis_attention_map
    ut2i.vis_attention_map = recorder
    try:
        B = x.shape[0]
        with torch.no_grad():
            out, _ = m(x, expand_t(T_VIS, B), context=ctx, dissect_name="p2p", fm_direction="decode", t_edit=t_edit, block_id="all",
                       token_kwargs=dict(token_dissect="p2p_rescale", p2p_multiplier=3.0),
                       target_context_ids=[a.copy() for a in IDS[:B]], vis_am_path="unused", caption_list=["p"] * B)
    finally:
        ut2i.vis_attention_map = orig
    return maps, out.numpy()


def main():
    import importlib
    _, uvit_t2i = _refshim.load_reference()
    ut2i = importlib.import_module("tools.utils_t2i")
    torch.set_grad_enabled(False)
    out = {}
    meta = dict(t=T_VIS, t_edit_live=0.5, t_edit_plain=0.1, multiplier=3.0, ids=[a.tolist() for a in IDS], S_blocks=list(S_BLOCKS),
                torch=torch.__version__)

    z = np.load(os.path.join(HERE, "tiny_t2i.npz"))
    m = uvit_t2i.UViT(clip_dim=64, num_clip_token=N_CTX, **TINY).eval()
    m.load_state_dict({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}, strict=True)
    x, ctx = torch.from_numpy(z["x"]), torch.from_numpy(z["ctx"])
    edit, o_edit = record(ut2i, m, x, ctx, 0.5)
    plain, o_plain = record(ut2i, m, x, ctx, 0.1)
    assert len(edit) == len(plain) == TINY["depth"] + 1
    diff = [float(np.abs(a - b).max()) for a, b in zip(edit, plain)]
    assert diff[0] == 0.0 and all(d > 0.0 for d in diff[1:]) and np.abs(o_edit - o_plain).max() > 0.0, diff
    for i, (a, b) in enumerate(zip(edit, plain)):
        out[f"tiny_edit/{i}"], out[f"tiny_plain/{i}"] = a, b
    out["tiny_block_diff"] = np.array(diff, np.float64)

    zb = np.load(os.path.join(HERE, "big_S_t.npz"))
    big_meta = json.loads(bytes(zb["meta_json"]).decode())
    torch.manual_seed(WEIGHT_SEED)
    m = uvit_t2i.UViT(clip_dim=768, num_clip_token=N_CTX, **COMMON, **SHAPES["S"]).eval()
    assert sd_sha256(m) == big_meta["sha256"], "the seeded U-ViT-S T2I is not the network of big_S_t.npz"
    x, ctx = torch.from_numpy(zb["x"]), torch.from_numpy(zb["ctx"])
    edit, _ = record(ut2i, m, x, ctx, 0.5)
    plain, _ = record(ut2i, m, x, ctx, 0.1)
    diff = [float(np.abs(a - b).max()) for a, b in zip(edit, plain)]
    assert diff[0] == 0.0 and all(d > 0.0 for d in diff[1:]), diff
    for i in S_BLOCKS:
        out[f"S_edit/{i}"] = edit[i]
    out["S_block_diff"] = np.array(diff, np.float64)
    meta["S_sha256"] = big_meta["sha256"]
    out["meta_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "attn_maps_t2i.npz")
    np.savez(path, **out)
    print(f"wrote attn_maps_t2i.npz: {os.path.getsize(path) / 1024:.1f} KiB; tiny diff {out['tiny_block_diff']}, S diff {diff}")


if __name__ == "__main__":
    main()
