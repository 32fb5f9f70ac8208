"""What the metric tools share on the host: the device rule, ``save_image``'s rounding, and how an image folder is listed, paired
with another and read.  ``fid_score`` re-exports ``IMAGE_EXTENSIONS``, ``ImagePathDataset``, ``MAX_WORKERS`` and ``_batches``
(they mirror the reference's tools/fid_score.py).  Neither Inception nor any other model is imported here, so a tool needs
``fid_score`` only for FID itself."""
import os
import pathlib

import numpy as np
import torch
from PIL import Image

from uspace_amd import _hip

try:
    from tqdm import tqdm
except ImportError:
    def tqdm(x):
        return x

IMAGE_EXTENSIONS = {"bmp", "jpg", "jpeg", "pgm", "png", "ppm", "tif", "tiff", "webp"}
MAX_WORKERS = 16


def rocm_device(device, what):
    """``torch.device(device)``; None means the ROCm device, and ``UspaceHipError`` naming ``what`` where there is none."""
    if device is None:
        if not torch.cuda.is_available():
            raise _hip.UspaceHipError(f"{what} needs a ROCm device (MI355X); uspace_amd has no CPU path")
        return torch.device("cuda")
    return torch.device(device)


def quantize(x):
    """``save_image``'s rounding of an fp32 tensor in [0, 1], x * 255 + 0.5 -> clamp -> uint8, then / 255: the numbers of the
    written PNG read back (``x`` is left as it is: the in-place steps act on ``mul``'s result).  On decoded bytes it is the
    identity on the byte, exactly: fl(255 fl(q / 255)) + 0.5 floors to q, whereas the product alone misses q by an ulp for some q
    where the level was formed with fl(1 / 255), as a device forms it.  The towers' preprocess kernels do this rounding
    themselves under ``quantize=True``; that is why ``cmmd`` passes it for a folder (the bits ``CMMD.update`` gives on the samples)
    while the ``dino_metrics``, ``id_metrics`` and ``pair_metrics`` folder paths pass ``quantize=False``."""
    return x.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).float() / 255


def require_paths(paths):
    for p in paths:
        if not os.path.exists(p):
            raise RuntimeError("Invalid path: %s" % p)


def image_files(path):
    """The image files of a folder in the reference's order: the per-extension globs, concatenated and sorted."""
    return sorted(file for ext in IMAGE_EXTENSIONS for file in pathlib.Path(path).glob(f"*.{ext}"))


def paired_image_files(dir_a, dir_b):
    """(names, files_a, files_b) of two folders paired by file name without its extension, sorted by name.  A name present in one
    folder only, or an image whose size differs from its partner's or from the first pair's, raises ValueError."""
    fa, fb = ({f.stem: f for f in image_files(d)} for d in (dir_a, dir_b))
    only = sorted(set(fa) ^ set(fb))
    if only or not fa:
        raise ValueError(f"the folders do not pair up by file name: {only[:8] if only else 'no images'}")
    names = sorted(fa)
    first = None
    for n in names:
        with Image.open(fa[n]) as ia, Image.open(fb[n]) as ib:
            first = first or ia.size
            if ia.size != ib.size or ia.size != first:
                raise ValueError(f"image sizes differ at {n!r}: {ia.size} and {ib.size} (the first pair is {first})")
    return names, [fa[n] for n in names], [fb[n] for n in names]


class ImagePathDataset(torch.utils.data.Dataset):
    """Images as uint8 [3, H, W] tensors (RGB)."""

    def __init__(self, files, transforms=None):
        self.files = files
        self.transforms = transforms

    def __len__(self):
        return len(self.files)

    def __getitem__(self, i):
        img = Image.open(self.files[i]).convert("RGB")
        if self.transforms is not None:
            return self.transforms(img)
        return torch.from_numpy(np.array(img, dtype=np.uint8)).permute(2, 0, 1).contiguous()


def _batches(files, batch_size, num_workers):
    """(batch_size, DataLoader) as the reference reads a folder: in order, the last batch ragged, ``batch_size`` capped at the
    number of files."""
    if batch_size > len(files):
        print("Warning: batch size is bigger than the data size. Setting batch size to data size")
        batch_size = len(files)
    loader = torch.utils.data.DataLoader(ImagePathDataset(files), batch_size=batch_size, shuffle=False, drop_last=False,
                                         num_workers=min(int(num_workers), MAX_WORKERS))
    return batch_size, loader


def unit_batches(files, batch_size, num_workers, device):
    """The batches of ``_batches`` as fp32 [b, 3, H, W] in [0, 1] on ``device`` (what ``transforms.ToTensor`` gives), with a
    progress bar where tqdm is installed."""
    for batch in tqdm(_batches(files, batch_size, num_workers)[1]):
        yield batch.to(device).float() / 255


def uint8_batches(files, batch_size):
    """uint8 [b, 3, H, W] host tensors of (equally sized) image files, in order, ``batch_size`` at a time, the last batch ragged."""
    data = ImagePathDataset(files)
    for lo in range(0, len(files), batch_size):
        yield torch.stack([data[i] for i in range(lo, min(lo + batch_size, len(files)))])


@torch.no_grad()
def chunked_features(fn, images, chunk, dims):
    """fp32 [B, dims]: ``fn`` of device images [B, ...], ``chunk`` of them at a time (a row must not depend on its chunk)."""
    _hip.require_device(images, "images")
    out = torch.empty(images.shape[0], dims, dtype=torch.float32, device=images.device)
    for lo in range(0, images.shape[0], chunk):
        out[lo:lo + chunk] = fn(images[lo:lo + chunk])
    return out
