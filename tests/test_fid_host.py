"""FID host side (no GPU): the Frechet distance against the reference's own results (tests/golden/fid_frechet.npz, made by
tests/golden/make_fid_golden.py), the Inception state_dict layout and loading rules, the finalisation of the shifted fp64
sums, and the new kernels' resources."""
import os

import numpy as np
import pytest
import torch

from uspace_amd.tools import fid_score, inception


def _golden(golden_dir):
    return np.load(os.path.join(golden_dir, "fid_frechet.npz"))


@pytest.mark.parametrize("case", ["small", "singular"])
def test_frechet_distance_matches_reference(golden_dir, case, capsys):
    z = _golden(golden_dir)
    assert not bool(z[f"{case}/raises"])
    got = fid_score.calculate_frechet_distance(z[f"{case}/mu1"], z[f"{case}/sigma1"], z[f"{case}/mu2"], z[f"{case}/sigma2"])
    want = float(z[f"{case}/fid"])
    assert abs(got - want) <= 1e-10 * abs(want), (got, want)
    retried = "singular product" in capsys.readouterr().out
    assert retried == (case == "singular")


def test_frechet_distance_raises_on_imaginary_component(golden_dir):
    z = _golden(golden_dir)
    assert bool(z["imaginary/raises"])
    with pytest.raises(ValueError, match="Imaginary component") as e:
        fid_score.calculate_frechet_distance(z["imaginary/mu1"], z["imaginary/sigma1"], z["imaginary/mu2"],
                                             z["imaginary/sigma2"])
    got = float(str(e.value).split()[-1])
    assert abs(got - float(z["imaginary/fid"])) <= 1e-10 * abs(float(z["imaginary/fid"]))


TABLE = {  # block -> (number of BasicConv2d, output channels at 299^2)
    "Conv2d_1a_3x3": (1, 32), "Conv2d_2a_3x3": (1, 32), "Conv2d_2b_3x3": (1, 64), "Conv2d_3b_1x1": (1, 80),
    "Conv2d_4a_3x3": (1, 192), "Mixed_5b": (7, 256), "Mixed_5c": (7, 288), "Mixed_5d": (7, 288), "Mixed_6a": (4, 768),
    "Mixed_6b": (10, 768), "Mixed_6c": (10, 768), "Mixed_6d": (10, 768), "Mixed_6e": (10, 768), "Mixed_7a": (6, 1280),
    "Mixed_7b": (9, 2048), "Mixed_7c": (9, 2048),
}
CONCAT_LAST = {"Mixed_5b": ["branch1x1", "branch5x5_2", "branch3x3dbl_3", "branch_pool"],
               "Mixed_6b": ["branch1x1", "branch7x7_3", "branch7x7dbl_5", "branch_pool"],
               "Mixed_7b": ["branch1x1", "branch3x3_2a", "branch3x3_2b", "branch3x3dbl_3a", "branch3x3dbl_3b", "branch_pool"]}


def test_state_dict_layout_is_torchvision_inception3():
    m = inception.InceptionV3(seed=0)
    sd = m.state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == inception.state_dict_layout()
    assert len(sd) == 94 * 5
    blocks = {}
    for k in sd:
        if k.endswith(".conv.weight"):
            blocks.setdefault(k.split(".")[0], []).append(k)
    assert list(blocks) == list(TABLE)
    for blk, (n, _c) in TABLE.items():
        assert len(blocks[blk]) == n, blk
    # FLOP count of the table at 299^2 (2 * MACs): 11.42 GFLOP per image
    flop, shapes = 0, inception.STAGE_SHAPES
    hw = {"Conv2d_1a_3x3": 149, "Conv2d_2a_3x3": 147, "Conv2d_2b_3x3": 147, "Conv2d_3b_1x1": 73, "Conv2d_4a_3x3": 71}
    for name, ci, co, (kh, kw), s, p in inception.ARCH:
        blk = name.split(".")[0]
        if blk in hw:
            h = w = hw[blk]
        else:
            src = {"Mixed_5": 35, "Mixed_6": 35 if blk == "Mixed_6a" else 17, "Mixed_7": 17 if blk == "Mixed_7a" else 8}[blk[:7]]
            h = (src + 2 * p[0] - kh) // s + 1 if "dbl_1" not in name else src
            w = (src + 2 * p[1] - kw) // s + 1
            if blk in ("Mixed_6a", "Mixed_7a") and s == 1:
                h, w = src, src
        flop += 2 * ci * co * kh * kw * h * w
    assert abs(flop / 1e9 - inception.GFLOP_PER_IMAGE) < 0.01, flop / 1e9
    assert [c for (_h, _w, c) in shapes[8:19]] == [256, 288, 288, 768, 768, 768, 768, 768, 1280, 2048, 2048]
    for blk, names in CONCAT_LAST.items():
        got = sum(sd[f"{blk}.{n}.conv.weight"].shape[0] for n in names)
        assert got == TABLE[blk][1], blk


def _write_checkpoint(path, extra=True, rename=None):
    sd = dict(inception.InceptionV3(seed=3).state_dict())
    if extra:
        for k in list(sd):
            if k.endswith(".bn.running_var"):
                sd[k.replace("running_var", "num_batches_tracked")] = torch.tensor(0)
        sd["fc.weight"] = torch.zeros(1008, 2048)
        sd["fc.bias"] = torch.zeros(1008)
    if rename:
        sd[rename[1]] = sd.pop(rename[0])
    torch.save(sd, path)
    return sd


def test_weight_file_with_fc_and_num_batches_tracked_loads(tmp_path):
    p = str(tmp_path / "w.pth")
    sd = _write_checkpoint(p)
    m = inception.InceptionV3(weights=p)
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k
    _write_checkpoint(p, extra=False)
    inception.InceptionV3(weights=p)


def test_renamed_key_raises_and_names_it(tmp_path):
    p = str(tmp_path / "w.pth")
    _write_checkpoint(p, rename=("Mixed_6c.branch7x7dbl_4.bn.running_mean", "Mixed_6c.branch7x7dbl_4.bn.running_avg"))
    with pytest.raises(KeyError) as e:
        inception.InceptionV3(weights=p)
    assert "Mixed_6c.branch7x7dbl_4.bn.running_mean" in str(e.value)
    assert "Mixed_6c.branch7x7dbl_4.bn.running_avg" in str(e.value)


def test_missing_weights_raise_without_download(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.hub, "get_dir", lambda: str(tmp_path))

    def no_network(*a, **k):
        raise AssertionError("network access attempted")
    monkeypatch.setattr(torch.hub, "load_state_dict_from_url", no_network)
    monkeypatch.setattr(torch.hub, "download_url_to_file", no_network)
    with pytest.raises(FileNotFoundError) as e:
        inception.InceptionV3()
    msg = str(e.value)
    assert os.path.join(str(tmp_path), "checkpoints") in msg and inception.FID_WEIGHTS_FILE in msg


def test_non_default_options_are_not_implemented():
    for kw in (dict(resize_input=False), dict(normalize_input=False), dict(use_fid_inception=False)):
        with pytest.raises(NotImplementedError):
            inception.InceptionV3(seed=0, **kw)


def test_statistics_finalisation_equals_np_cov_with_large_offset():
    rng = np.random.default_rng(5)
    x = (1e3 + rng.standard_normal((500, 64))).astype(np.float32).astype(np.float64)
    n = len(x)
    c = x[:50].mean(0)                                  # the first batch's mean
    s1 = np.zeros(64)
    s2 = np.zeros((64, 64))
    for lo in range(0, n, 50):
        d = x[lo:lo + 50] - c
        s1 += d.sum(0)
        s2 += d.T @ d
    mu, sigma = fid_score.finalize_statistics(n, c, s1, s2)
    ref_mu, ref_sigma = x.mean(0), np.cov(x, rowvar=False)
    assert np.linalg.norm(mu - ref_mu) / np.linalg.norm(ref_mu) < 1e-10
    assert np.linalg.norm(sigma - ref_sigma) / np.linalg.norm(ref_sigma) < 1e-10


def test_image_files_are_read_and_sorted_as_the_reference_does(tmp_path):
    from PIL import Image
    names = ["10.png", "2.png", "1.jpg", "a.webp", "skip.txt"]
    for i, nm in enumerate(names[:-1]):
        Image.fromarray(np.full((4, 5, 3), i * 40, np.uint8)).save(tmp_path / nm)
    (tmp_path / names[-1]).write_text("x")
    import pathlib
    files = sorted([f for ext in fid_score.IMAGE_EXTENSIONS for f in pathlib.Path(tmp_path).glob(f"*.{ext}")])
    assert [f.name for f in files] == ["1.jpg", "10.png", "2.png", "a.webp"]
    ds = fid_score.ImagePathDataset(files)
    t = ds[1]
    assert t.dtype == torch.uint8 and tuple(t.shape) == (3, 4, 5) and int(t[0, 0, 0]) == 0


def test_new_kernels_use_no_scratch():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(root, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    ks = kr.kernels()
    names = dict(zip([k["name"] for k in ks], kr.demangle([k["name"] for k in ks])))
    mine = [k for k in ks if any(s in names[k["name"]] for s in ("conv_kernel", "pool3_kernel", "resize_input_kernel",
                                                                "spatial_mean_kernel", "stats_s1_kernel", "stats_s2_kernel",
                                                                "pack_conv_kernel"))]
    assert len(mine) >= 9, [names[k["name"]] for k in mine]
    for k in mine:
        assert k["scratch"] == 0, names[k["name"]]
