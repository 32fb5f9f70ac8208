"""What every model wrapper keeps on the device besides its parameters: the weights packed into the kernel layout by the
library's ``{prefix}pack_weights`` (PackedWeights) and the workspaces its launches run in (WorkspaceCache)."""
import ctypes

import torch

from . import _hip


class PackedWeights:
    """The blob of one model (or one half of it), repacked when a tensor changed.  ``prefix``: the library's symbol prefix
    (``"uspace_uvit_"``); ``name``: the model's name in error messages; ``tensors``: callable returning the tensors in the
    library's canonical order; ``cfg``: the config struct every entry point of the family takes first (None: it takes none; an
    int: the family takes that int first, by value -- ``uspace_lpips_``'s ``net``)."""

    def __init__(self, prefix, name, tensors, cfg=None):
        self.prefix, self.name, self.tensors, self.cfg = prefix, name, tensors, cfg
        self._held = None          # (device, versions, blob)

    def invalidate(self):
        """Needed only after IN-PLACE edits through ``p.data`` (``p.data.copy_(w)``, ``p.data.mul_()``), which change neither the
        tensor's version counter nor its storage -- the two things ``blob`` watches; ``load_state_dict``, ``.to()``, optimiser
        steps and plain in-place ops on the parameter are picked up by itself."""
        self._held = None

    def blob(self, device):
        ts = self.tensors()
        versions = tuple((t.data_ptr(), t._version) for t in ts)
        if self._held is not None and self._held[0] == device and self._held[1] == versions:
            return self._held[2]
        L = _hip.lib()
        lead = () if self.cfg is None else (self.cfg if isinstance(self.cfg, int) else ctypes.byref(self.cfg),)
        n = getattr(L, self.prefix + "num_params")(*lead)
        if n != len(ts):
            raise _hip.UspaceHipError(f"{self.name} parameter count mismatch: module {len(ts)} vs library {n}")
        srcs = []
        for i, t in enumerate(ts):
            _hip.require_device(t, f"{self.name} parameter")
            want = getattr(L, self.prefix + "param_numel")(*lead, i)
            if t.numel() != want:
                raise _hip.UspaceHipError(f"{self.name} parameter {i}: shape {tuple(t.shape)} has {t.numel()} elements, the library expects {want}")
            srcs.append(t.detach().to(torch.float32).contiguous())
        nbytes = getattr(L, self.prefix + "weight_bytes")(*lead)
        blob = torch.empty(nbytes, dtype=torch.uint8, device=device)
        arr = (ctypes.c_void_p * n)(*[s.data_ptr() for s in srcs])
        _hip.check(getattr(L, self.prefix + "pack_weights")(*lead, arr, n, _hip.ptr(blob), nbytes, _hip.stream_ptr()),
                   self.prefix + "pack_weights")
        _hip.sync_current_stream()   # srcs may be temporaries
        self._held = (device, versions, blob)
        return blob


class WorkspaceCache(dict):
    """(batch or chunk size, device) -> uint8 workspace: at most ``slots`` entries, the most recently used last."""

    def __init__(self, slots):
        super().__init__()
        self.slots = slots

    def take(self, B, device, nbytes):
        """The workspace for ``B`` on ``device``, of ``nbytes`` bytes at least.  The caller asks the library for ``nbytes`` every
        time: the size depends on the library's process-wide switches (``uspace_gemm_set_sk``) and, for some models, on more than
        ``B``, and a workspace sized for less must not be handed on.  A new entry evicts the least recently used."""
        key = (B, str(device))
        ws = self.pop(key, None)
        if ws is None or ws.numel() < nbytes:
            while len(self) >= self.slots:
                self.pop(next(iter(self)))          # dicts keep insertion order: the oldest use
            ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self[key] = ws
        return ws
