"""What the towers of libs/clip.py and libs/dino.py share on the host: the packed blob and the workspace cache (``_Tower``) and, for
the image towers, preprocessing, the check of ``pixel_values``, the ``hidden_state`` -> stop mapping and the outputs (``_ImageTower``).
A subclass names its library symbols (``_SYMBOLS``) and itself (``_DISPLAY``), supplies ``_c_cfg()`` and calls ``_finish_init()``."""
import ctypes

import torch
import torch.nn as nn

from .. import _hip
from .._blob import PackedWeights, WorkspaceCache


class _Tower(nn.Module):
    _SYMBOLS = _DISPLAY = None

    def _finish_init(self):
        self._packed = PackedWeights(self._SYMBOLS, self._DISPLAY, self._canonical_params, self._c_cfg())
        self._ws = WorkspaceCache(1)
        self.eval()
        self.requires_grad_(False)

    def invalidate_packed(self):
        """Forget the packed weight blob; needed only after in-place edits through ``p.data`` (``PackedWeights.invalidate``)."""
        self._packed.invalidate()

    def _canonical_params(self):
        return list(self.parameters())

    def _packed_blob(self, device):
        return self._packed.blob(device)

    def _forward_args(self, B, dev):
        """-> (library, what every forward takes first: config, blob, workspace, its bytes); the caches keep blob and workspace alive."""
        blob = self._packed_blob(dev)
        L = _hip.lib()
        cfg = self._c_cfg()
        ws = self._ws.take(B, dev, getattr(L, self._SYMBOLS + "workspace_bytes")(ctypes.byref(cfg), B))
        return L, (ctypes.byref(cfg), _hip.ptr(blob), _hip.ptr(ws), ws.numel())


class _ImageTower(_Tower):
    """A tower over ``pixel_values`` [B, 3, S, S]; ``cfg`` holds ``image`` and ``dim``, ``tokens`` the sequence length."""

    def _preprocess(self, images, quantize, mean, std):
        _hip.require_device(images, "images")
        if images.dim() != 4 or images.shape[1] != 3 or images.shape[2] != images.shape[3]:
            raise ValueError(f"images must be [B, 3, H, H] (square), got {tuple(images.shape)}")
        S = self.cfg["image"]
        x = images.detach().to(torch.float32).contiguous()
        B, _, H, W = x.shape
        out = torch.empty(B, 3, S, S, dtype=torch.float32, device=x.device)
        if B == 0:
            return out
        m3, s3 = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
        _hip.check(_hip.lib().uspace_clip_preprocess(_hip.ptr(x), _hip.ptr(out), B, H, W, S, 1 if quantize else 0, m3, s3,
                                                     _hip.stream_ptr()), "uspace_clip_preprocess")
        return out

    def _check_pixel_values(self, pixel_values):
        """-> B of pixel_values [B, 3, S, S] on the device."""
        _hip.require_device(pixel_values, "pixel_values")
        S = self.cfg["image"]
        if pixel_values.dim() != 4 or tuple(pixel_values.shape[1:]) != (3, S, S):
            raise ValueError(f"pixel_values must be [B, 3, {S}, {S}], got {tuple(pixel_values.shape)}")
        return pixel_values.shape[0]

    @staticmethod
    def _stop(hidden_state):
        """``stop_after_layer`` of the forwards: None -> -1 (the whole model), "embeddings" -> -2, a layer count k -> k."""
        stop = -1 if hidden_state is None else (-2 if hidden_state == "embeddings" else int(hidden_state))
        if stop < -2:
            raise ValueError("hidden_state must be None, 'embeddings' or a layer count >= 0")
        return stop

    def _out(self, pixel_values, *shape, dtype=torch.float32):
        """An output [B, *shape] on the device of ``pixel_values``."""
        return torch.empty(pixel_values.shape[0], *shape, dtype=dtype, device=pixel_values.device)
