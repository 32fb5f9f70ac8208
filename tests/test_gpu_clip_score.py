"""``CLIPScore`` (uspace_amd/tools/clip_score.py) on the GPU with the tiny towers of tests/golden/clip_vision_tiny.npz and a stub
tokenizer, against the float64 pipeline of tests/clip_vision_cases.py: per-sample scores from images in [0, 1], the running mean
over two updates, the directional similarity, and a matched (image, prompt) assignment scoring above the swapped one."""
import pytest
import torch

from tests import clip_vision_cases as C

pytestmark = pytest.mark.gpu

PROMPTS = ["a photo of a cat", "two dogs on a red sofa in the evening light", "mountains", "a", "blue car street",
           "an astronaut riding a horse on the moon"]


@pytest.fixture(scope="module")
def rig():
    """The metric on the device and the float64 pipeline's embeddings of 6 images and 6 prompts, computed once."""
    from uspace_amd.libs.clip import CLIPTextProjection, CLIPTextTransformer, CLIPVisionTransformer
    from uspace_amd.tools.clip_score import CLIPScore
    n = C.S.cpu_threads()
    z, sd = C.load_golden()
    vision, text, proj = CLIPVisionTransformer(**C.TINY_VISION), CLIPTextTransformer(**C.TINY_TEXT), CLIPTextProjection(128, 64)
    for m in (vision, text, proj):
        m.load_state_dict(sd)
    tok = C.StubTokenizer()
    metric = CLIPScore(vision, text, proj, tok, device="cuda")
    images = C.make_images(6, 64, seed=9, kind="mixed")
    ids = tok(PROMPTS)["input_ids"]
    e_img = C.vision_forward(C.preprocess(images, 56), sd, 2, "loose")["image_embeds"]
    e_txt = C.text_embeds(C.text_forward(ids, sd, 2), ids, sd["text_projection.weight"])
    yield dict(metric=metric, images=images, e_img=e_img, e_txt=e_txt)
    torch.set_num_threads(n)


def test_update_and_compute_against_the_float64_pipeline(rig):
    metric, images = rig["metric"], rig["images"]
    metric.reset()
    ref = C.clip_score(rig["e_img"], rig["e_txt"])
    s1 = metric.update(images[:4].cuda(), PROMPTS[:4])
    s2 = metric.update(images[4:].cuda(), PROMPTS[4:])
    got = torch.cat([s1, s2]).cpu()
    assert got.dtype == torch.float32 and s1.is_cuda and metric.count == 6 and metric.score_sum.dtype == torch.float64
    e = C.maxabs(got, ref)
    e_feat = max(C.rel(metric.image_features(images.cuda()).cpu(), rig["e_img"]), C.rel(metric.text_features(PROMPTS).cpu(), rig["e_txt"]))
    e_raw = C.maxabs(metric.similarity(metric.image_features(images.cuda()), metric.text_features(PROMPTS)).cpu(),
                     C.cosine(rig["e_img"], rig["e_txt"]))
    print(f"scores {['%.3f' % v for v in got.tolist()]}: max abs error {e:.2e} (of 100); features rel {e_feat:.2e}; raw cosine {e_raw:.2e}")
    assert e < C.TOL["score"] and e_raw < C.TOL["cosine"]
    assert abs(metric.compute() - float(got.double().mean())) < 1e-12
    assert abs(metric.compute() - float(ref.mean())) < C.TOL["score"]
    metric.reset()
    assert metric.count == 0
    with pytest.raises(ValueError):
        metric.compute()
    # an empty update changes nothing and returns an empty tensor
    assert metric.update(torch.empty(0, 3, 64, 64, device="cuda"), []).shape == (0,) and metric.count == 0


def test_scores_follow_the_prompts_and_a_matched_assignment_wins(rig):
    """Permuting the prompts gives the scores of the permuted pairs; and of two images and two prompts chosen on the float64 cosine
    matrix so that the matched assignment (a, p0), (b, p1) beats the swapped one, the GPU ranks them the same way."""
    metric, images = rig["metric"], rig["images"]
    cos = C.cosine(rig["e_img"][:, None], rig["e_txt"][None])              # [6 images, 6 prompts]
    perm = [3, 0, 5, 1, 2, 4]
    got = metric.update(images.cuda(), [PROMPTS[j] for j in perm]).cpu()
    assert C.maxabs(got, 100.0 * cos[torch.arange(6), perm].clamp_min(0.0)) < C.TOL["score"]
    # image a: the one that prefers prompt 0 over prompt 1 most; image b: the one that prefers it least
    pref = cos[:, 0] - cos[:, 1]
    a, b = int(pref.argmax()), int(pref.argmin())
    margin = 100.0 * float(pref[a] - pref[b])
    # four scores enter the comparison, each within TOL["score"] of its float64 value
    assert margin > 4.0 * C.TOL["score"], "the seeded images do not separate the two assignments"
    pair = images[[a, b]].cuda()
    matched = metric.update(pair, [PROMPTS[0], PROMPTS[1]]).double().sum()
    swapped = metric.update(pair, [PROMPTS[1], PROMPTS[0]]).double().sum()
    print(f"matched {float(matched):.3f} swapped {float(swapped):.3f} (float64 margin {margin:.3f})")
    assert float(matched) > float(swapped)
    metric.reset()


def test_directional_similarity(rig):
    metric, images = rig["metric"], rig["images"]
    src, edit = images[:3], images[3:]
    ref = C.directional(rig["e_img"][:3], rig["e_img"][3:], rig["e_txt"][:3], rig["e_txt"][3:])
    got = metric.directional_similarity(src.cuda(), edit.cuda(), PROMPTS[:3], PROMPTS[3:]).cpu()
    e = C.maxabs(got, ref)
    print(f"directional similarity {got.tolist()} vs {ref.tolist()}: max abs {e:.2e}")
    assert e < C.TOL["directional"]
    assert got.shape == (3,)


def test_host_tensors_are_refused(rig):
    from uspace_amd import _hip
    with pytest.raises(_hip.UspaceHipError):
        rig["metric"].update(rig["images"][:1], PROMPTS[:1])
    with pytest.raises(ValueError):
        rig["metric"].update(rig["images"][:2].cuda(), PROMPTS[:1])
