"""Host-side logic of the T2I attention-map edit (reference: tools/utils_t2i.py:196-296).

The reference materialises softmax(QK^T) [B,H,L,L], multiplies the columns of the target
context tokens, and multiplies by V.  Because the edit happens after softmax with no
renormalisation, (P * colscale) @ V == P @ (diag(colscale) V): the HIP attention kernel takes
a per-(batch, key) factor table instead, and never materialises the map.  This file only
decides WHICH factors apply at a given step / block (same control flow as the reference).
"""
import numpy as np

TIME_TOKEN_NUM = 1
EDIT_NAMES = ("p2p", "local_prompt", "sampled_image_editing")


def uses_attention_edit_path(kwargs):
    """libs/uvit_t2i.py:91-96: these dissect names route attention through the editable map."""
    return kwargs.get("dissect_name") in EDIT_NAMES


def block_selected(target_block_id, block_id):
    """tools/utils_t2i.py:227-238."""
    if isinstance(target_block_id, (int, np.integer)) and not isinstance(target_block_id, bool):
        return block_id == int(target_block_id)
    if isinstance(target_block_id, (list, tuple)):
        return block_id in target_block_id
    if isinstance(target_block_id, str) and target_block_id == "all":
        return True
    if target_block_id is None:
        return True
    raise ValueError(f"unknown target_block_id {target_block_id}")


def key_scale_table(n_blocks, B, L, timestep_digit, kwargs):
    """[n_blocks, B, L] fp32 factors (1 = untouched) or None when this step edits nothing.

    Error behaviour follows the reference: ValueError for a foreign dissect_name,
    NotImplementedError for an unknown fm_direction / token_dissect."""
    name = kwargs.get("dissect_name")
    if name not in EDIT_NAMES:
        raise ValueError(f"dissect_name should be read or write, here is {name}")
    direction = kwargs.get("fm_direction")
    if direction == "encode":
        return None
    if direction != "decode":
        raise NotImplementedError(f"fm_direction={direction}")
    if not float(timestep_digit) <= kwargs.get("t_edit"):
        return None
    tk = kwargs["token_kwargs"]
    mode = tk["token_dissect"]
    if mode.startswith("lp_"):
        return None
    if mode != "p2p_rescale":
        raise NotImplementedError(mode)
    ids = kwargs["target_context_ids"]
    mult = tk["p2p_multiplier"]
    if isinstance(mult, (int, float)):
        mult = [mult] * len(ids)
    elif not isinstance(mult, list):
        raise ValueError(f"unknown p2p_multiplier {mult}")
    row = np.ones((B, L), np.float32)
    touched = False
    for b, tid in enumerate(ids):
        tid = np.asarray(tid)
        if tid.size > 0:
            row[b, tid.astype(np.int64) + TIME_TOKEN_NUM] = np.float32(mult[b])
            touched = True
    table = np.ones((n_blocks, B, L), np.float32)
    any_block = False
    for blk in range(n_blocks):
        if block_selected(kwargs.get("block_id"), blk):
            table[blk] = row
            any_block = True
    if not (touched and any_block):
        return None
    return table


# ------------------------------------------------------------------------------------------------ the map itself
# tools/utils_t2i.py:141-193 vis_attention_map: at these timestep digits the reference writes, per prompt and block, the head-mean
# image-token x text-token map as one row of heat tiles.  Here the map comes from uspace_attention_map_bf16 (the fused attention
# kernel never holds it); this part lays it out and writes the PNGs.
VIS_DIGITS = ("0.10", "0.20", "0.30", "0.40", "0.50", "0.60", "0.70", "0.80", "0.90")
LABEL_RATIO = 0.2        # height of the label strip under a tile, of the tile's height (ptp_utils.text_under_image)
GAP_RATIO = 0.02         # white gap between two tiles, of the labelled tile's height (ptp_utils.view_images)

_TOKENIZER = None


def token_range(name, num_clip_token, num_patches):
    """(first token, count) of a named token group in the T2I order time (1), context (num_clip_token), image (num_patches);
    an explicit (first, count) pair passes through after a range check."""
    L = TIME_TOKEN_NUM + num_clip_token + num_patches
    if isinstance(name, str):
        table = {"time": (0, TIME_TOKEN_NUM), "context": (TIME_TOKEN_NUM, num_clip_token),
                 "image": (TIME_TOKEN_NUM + num_clip_token, num_patches), "all": (0, L)}
        if name not in table:
            raise ValueError(f"unknown token group {name!r}: one of {sorted(table)} or a (first, count) pair")
        return table[name]
    try:
        first, count = (int(v) for v in name)
    except (TypeError, ValueError):
        raise ValueError(f"token group must be a name or a (first, count) pair, got {name!r}")
    if first < 0 or count < 1 or first + count > L:
        raise ValueError(f"token range ({first}, {count}) does not lie inside the {L} tokens")
    return first, count


def default_tokenizer():
    """The CLIP tokenizer the reference names (tools/utils_t2i.py:153), loaded once per process (the reference reloads it on every
    call).  Nothing is downloaded here: Hugging Face raises what it raises if the files are not in its cache."""
    global _TOKENIZER
    if _TOKENIZER is None:
        from transformers import CLIPTokenizer
        _TOKENIZER = CLIPTokenizer.from_pretrained("openai/clip-vit-large-patch14")
    return _TOKENIZER


def cross_attention_tiles(map_b, grid, origin_size=256):
    """Heat tiles of one sample: map_b [grid * grid, n_tok] (image token x text token, head mean) -> uint8
    [n_tok, origin_size, origin_size, 3].  Per token 255 * m / m.max() in fp32, truncated to uint8, grey on three channels, resized
    with PIL's default resampling (tools/utils_t2i.py:176-183)."""
    from PIL import Image
    m = np.asarray(map_b, np.float32)
    if m.ndim != 2 or m.shape[0] != grid * grid:
        raise ValueError(f"map must be [{grid * grid}, n_tok], got {m.shape}")
    tiles = np.empty((m.shape[1], origin_size, origin_size, 3), np.uint8)
    for i in range(m.shape[1]):
        img = m[:, i].reshape(grid, grid)
        img = (np.float32(255) * img / img.max()).astype(np.uint8)
        img = np.repeat(img[:, :, None], 3, axis=2)
        tiles[i] = np.asarray(Image.fromarray(img).resize((origin_size, origin_size)))
    return tiles


def tile_offsets(n_tiles, origin_size=256):
    """(x of every tile, width, height) of the row image: tiles of origin_size with a label strip under each, white gaps between."""
    h = origin_size + int(origin_size * LABEL_RATIO)
    gap = int(h * GAP_RATIO)
    return [j * (origin_size + gap) for j in range(n_tiles)], origin_size * n_tiles + gap * (n_tiles - 1), h


def vis_attention_map(maps, timestep_digit, origin_size=256, grid=None, **kwargs):
    """maps [n_blocks, B, grid * grid, num_clip_token] (tensor or array): at the nine digits of VIS_DIGITS one PNG per prompt of
    ``kwargs["caption_list"]`` and block, ``{prompt}_block{block_id}_time{digit}.png`` under ``kwargs["vis_am_path"]`` (created if
    missing; a later evaluation with the same digit overwrites, as in the reference).  Column i of the map is shown under the label of
    token i of ``tokenizer.encode(prompt)`` (``kwargs["tokenizer"]`` or the cached CLIP tokenizer).  Returns the paths written.
    The labels are drawn with PIL (the reference: cv2.putText): their pixels are no part of any parity claim, the tiles are."""
    if timestep_digit not in VIS_DIGITS:
        return []
    import os
    from PIL import Image, ImageDraw
    path = kwargs.get("vis_am_path")
    if path is None:
        return []
    m = maps.detach().cpu().numpy() if hasattr(maps, "detach") else np.asarray(maps)
    n_blocks, B, n_img, n_ctx = m.shape
    if grid is None:
        grid = int(round(n_img ** 0.5))
    prompts = kwargs["caption_list"]
    if len(prompts) < B:
        raise ValueError(f"caption_list holds {len(prompts)} prompts for a batch of {B}")
    tokenizer = kwargs.get("tokenizer")
    if tokenizer is None:
        tokenizer = default_tokenizer()
    os.makedirs(path, exist_ok=True)
    written = []
    for b in range(B):
        tokens = list(tokenizer.encode(prompts[b]))
        if len(tokens) > n_ctx:
            raise ValueError(f"prompt {b} encodes to {len(tokens)} tokens, the map has {n_ctx} text columns")
        labels = [str(tokenizer.decode(int(t))) for t in tokens]
        xs, width, height = tile_offsets(len(tokens), origin_size)
        for blk in range(n_blocks):
            tiles = cross_attention_tiles(m[blk, b][:, :len(tokens)], grid, origin_size)
            row = np.full((height, width, 3), 255, np.uint8)
            for j, x0 in enumerate(xs):
                row[:origin_size, x0:x0 + origin_size] = tiles[j]
            img = Image.fromarray(row)
            draw = ImageDraw.Draw(img)
            for j, x0 in enumerate(xs):
                box = draw.textbbox((0, 0), labels[j])
                tw, th = box[2] - box[0], box[3] - box[1]
                draw.text((x0 + (origin_size - tw) // 2, origin_size + (height - origin_size - th) // 2), labels[j], fill=(0, 0, 0))
            out = os.path.join(path, f"{prompts[b]}_block{blk}_time{timestep_digit}.png")
            img.save(out)
            written.append(out)
    return written
