"""The calls whose raw output bytes pin the two streaming attention kernels bit for bit (a helper, not a test): the long form
(uspace_amd/csrc/attention_long.hip, uspace_attention_long_bf16: heads of 64, packed qkv, 64-key tiles) and the wide form
(uspace_amd/csrc/attention_wide.hip, uspace_attention_wide_bf16: one head of 64 .. 512 channels, 32-key tiles).  Shared by tests/golden/make_attention_stream_digests.py
(which records the sha256 of every output) and tests/test_gpu_attention_stream_bits.py (which compares).  Every call is run-to-run
bit-equal (tests/test_gpu_attention_long.py and tests/test_gpu_attention_wide.py assert it), and a row's bits depend on the key-tile
size and the order of the accumulations alone: a change of either kernel that keeps both -- their merge into one among them -- leaves
every digest as it is."""
import os

import torch

from tests import attention_cases as AC
from tests import attention_long_cases as LC
from tests import attention_wide_cases as WC
from tests.vit_tower_cases import digest

HERE = os.path.dirname(os.path.abspath(__file__))
DIGESTS = os.path.join(HERE, "golden", "attention_stream_digests.json")

# (B, H, L): QB 64; QB 128 with a ragged last query and key tile; the first length beyond the resident kernel; one key tile, and one
# key in the second tile; 18 key tiles.  Each with and without key_scale; data set 'edges' (rows that meet their maximum in the first
# and in the last key tile), 'workflow' at L = 1.
LONG_CALLS = ((2, 3, 401), (8, 16, 401), (1, 1, 337), (2, 2, 1), (1, 2, 65), (1, 1, 1102))
LONG_QB = {(2, 3, 401): 64, (8, 16, 401): 128}
N_WIDE = 129


def wide_calls():
    """(B, N, C): every width at (3, 129); C = 512 at one key and at one key in the second tile; the widest and the narrowest head
    under the plan's 2- and 4-wave branches."""
    bb = WC.branch_batches(N_WIDE)
    calls = [(3, N_WIDE, C) for C in WC.WIDTHS] + [(3, 1, 512), (3, 33, 512)]
    calls += [(bb[nw], N_WIDE, C) for C in (512, 64) for nw in (2, 4)]
    return calls


def long_outputs():
    from uspace_amd import _hip
    for B, H, L in LONG_CALLS:
        qkv = AC.make_qkv(B, L, H, "edges" if L > 3 else "workflow").cuda().reshape(B * L, -1)       # ('edges' plants keys 0 .. 3)
        for scaled in (False, True):
            if (B, H, L) in LONG_QB:
                assert LC.plan(B, L, H, scaled)[1] == LONG_QB[(B, H, L)]
            ks = AC.make_key_scale(B, L).cuda() if scaled else None
            yield f"{B}x{L}x{H}-{'ks' if scaled else 'plain'}", _hip.attention_long(qkv, B, L, H, key_scale=ks)


def wide_outputs():
    for B, N, C in wide_calls():
        q, k, v, scale = WC.make_qkv(B, N, C, "last")
        yield f"{B}x{N}x{C}-nw{WC.plan(B, N, C)[2]}", WC.run(q, k, v, B, N, C, scale)


# form -> generator of (call, output tensor)
CASES = {"long": long_outputs, "wide": wide_outputs}


def case_digests(case):
    """{call: sha256} of one form's calls, computed on the GPU."""
    out = {call: digest(t) for call, t in CASES[case]()}
    torch.cuda.synchronize()
    return out
