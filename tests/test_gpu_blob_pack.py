"""The packed weight blobs on the GPU: (1) the bytes ``uspace_*_pack_weights`` writes for the tiny models, as sha256 digests
against tests/golden/blob_digests.json (recorded by tests/golden/make_blob_golden.py at the commit named in the file; the blob is
zeroed first, so the padding is compared too); (2) one cache contract for all the wrappers: when the blob is reused, when it is
repacked, and how many workspaces stay resident."""
import ctypes
import json
import os

import pytest
import torch

from tests import blob_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tiny(golden_dir):
    return {kind: C.tiny_model(kind, golden_dir) for kind in C.TINY_KINDS}


@pytest.mark.parametrize("kind", C.TINY_KINDS)
def test_packed_bytes_equal_the_recorded_digest(golden_dir, tiny, kind):
    want = json.load(open(os.path.join(golden_dir, "blob_digests.json")))["digests"]
    _m, prefix, cfg, tensors = tiny[kind]
    assert C.blob_digest(prefix, cfg, tensors) == want[kind]


# kind -> (blob getter, workspace cache attribute, slots, one run at batch B)
def _uvit(m, B):
    m(torch.zeros(B, 4, 16, 16, device="cuda"), torch.tensor(0.5, device="cuda").expand(B), None, edit_loc=None)


WRAPPERS = {
    "tiny_u": ("_packed_blob", "_workspace", 2, _uvit),
    "vae": ("_packed_blob", "_ws", 1, lambda m, B: m.decode(torch.zeros(B, 4, m.z_res, m.z_res, device="cuda"))),
    "vae_enc": ("_packed_enc_blob", "_ws_enc", 1,
                lambda m, B: m.encode_moments(torch.zeros(B, 3, m.resolution, m.resolution, device="cuda"))),
    "clip": ("_packed_blob", "_ws", 1, lambda m, B: m(torch.zeros(B, 77, dtype=torch.long, device="cuda"))),
    "clipv": ("_packed_blob", "_ws", 1, lambda m, B: m(torch.zeros(B, 3, m.cfg["image"], m.cfg["image"], device="cuda"))),
    "inception": ("_blob", "_ws", 1, lambda m, B: m.features(torch.rand(B, 3, 64, 64, device="cuda"))),
    "lpips": ("_packed_blob", "_ws", 1, lambda m, B: m(torch.rand(B, 3, 64, 64, device="cuda"), torch.rand(B, 3, 64, 64, device="cuda"))),
    "dino": ("_packed_blob", "_ws", 1, lambda m, B: m(torch.zeros(B, 3, m.cfg["image"], m.cfg["image"], device="cuda"))),
    "arcface": ("_blob", "_ws", 2, lambda m, B: m(torch.zeros(B, 3, 32, 32, device="cuda"))),
}
TINY_OF = {"lpips": "lpips_alex", "arcface": "idnet"}      # the wrapper's tiny model where its kind is named otherwise


@pytest.mark.parametrize("kind", sorted(WRAPPERS))
def test_blob_and_workspace_cache_contract(tiny, kind):
    from uspace_amd._blob import WorkspaceCache
    getter, ws_attr, slots, run = WRAPPERS[kind]
    m, _prefix, _cfg, tensors = tiny[TINY_OF.get(kind, kind)]
    blob = getattr(m, getter)
    dev = torch.device("cuda", torch.cuda.current_device())
    p = tensors[0]
    m.invalidate_packed()
    a = blob(dev)
    assert blob(dev) is a                                  # nothing changed: the same blob object
    with torch.no_grad():
        p.add_(0)                                          # in place on the parameter: the version counter moves
    b = blob(dev)
    assert b is not a and blob(dev) is b
    p.data.add_(0)                                         # through .data: neither version nor storage moves
    assert blob(dev) is b
    m.invalidate_packed()
    c = blob(dev)
    assert c is not b
    # workspaces: at most `slots` resident; a second batch size evicts the first only where there is one slot
    cache = getattr(m, ws_attr)
    assert isinstance(cache, WorkspaceCache) and cache.slots == slots
    cache.clear()
    run(m, 2)
    (k2, ws2), = cache.items()
    assert k2 == (2, str(dev))
    run(m, 3)
    assert len(cache) <= slots and (3, str(dev)) in cache
    assert (cache.get(k2) is ws2) if slots == 2 else (k2 not in cache)
    run(m, 2)
    run(m, 4)
    assert len(cache) == slots and list(cache)[-1] == (4, str(dev))
    cache.clear()


def test_workspace_sized_without_the_k_split_tail_is_not_handed_on():
    """uspace_gemm_set_sk changes uspace_uvit_workspace_bytes (U-ViT-L at batch 8: the tail's slabs and counters): the cache asks
    for the size on every call, so the entry sized with the switch off is replaced, not handed out, once the switch is on."""
    from bench import COMMON, MODELS
    from uspace_amd import _hip
    from uspace_amd._blob import WorkspaceCache
    L = _hip.lib()
    cfg = C.uvit_cfg(**dict(COMMON, **MODELS["L_u"]))
    need = lambda: L.uspace_uvit_workspace_bytes(ctypes.byref(cfg), 8)
    cache = WorkspaceCache(2)
    try:
        assert L.uspace_gemm_set_sk(0) == 0
        small = cache.take(8, "cuda", need())
        assert cache.take(8, "cuda", need()) is small
        assert L.uspace_gemm_set_sk(1) == 0
        assert need() > small.numel()
        big = cache.take(8, "cuda", need())
        assert big is not small and big.numel() >= need() and list(cache.values()) == [big]
        assert L.uspace_gemm_set_sk(0) == 0
        assert cache.take(8, "cuda", need()) is big        # large enough for the smaller plan: kept
    finally:
        L.uspace_gemm_set_sk(-1)
