"""Cases, float64 model, plan mirror and faults for the few-keys / many-queries attention (uspace_amd/csrc/attention_kv.hip); a
helper of tests/test_attention_kv_host.py (CPU) and tests/test_gpu_attention_kv.py (GPU), not a test.

Bounds (``TOL``): 3 x the worst value an MI355X measured with THIS kernel over the 39 cases of ``cases()``, every head and every
query row, against the float64 model -- ``att_tight`` / ``att_loose`` per head against the model that rounds where the kernel rounds /
the plain float64 softmax, ``row_tight`` per query row -- and never above the resident kernel's own bound
(``attention_cases.TOL`` without key_scale), whose row arithmetic this kernel repeats bit for bit wherever both take a shape
(Lq == Lk; the GPU test shows it)."""
import numpy as np
import torch

from tests.attention_cases import TOL as RESIDENT_TOL

DH = 64
MEASURED = dict(
    att_tight=2.366e-4,     # B1-Lq17-Lk335-H8-voff
    att_loose=2.575e-3,     # B3-Lq1-Lk256-H8-workflow (3 x it is 7.7e-3: the resident kernel's 7.4e-3 is the smaller)
    row_tight=3.216e-3,     # B1-Lq1024-Lk256-H5-sharp
)
TOL = {k: min(RESIDENT_TOL[k], float(f"{3 * v:.2g}")) for k, v in MEASURED.items()}      # 7.1e-4, 7.4e-3, 9.6e-3
DATA_SETS = ("workflow", "flat", "sharp", "voff")

LK = (1, 12, 16, 17, 256, 335, 336)
LQ = (1, 15, 17, 825, 960)
HEADS = (1, 2, 3, 5, 8)
# the four stages of one 512^2 image: (Lq, H) at Lk = 256
WORKFLOW = ((16384, 1), (4096, 2), (1024, 5), (256, 8))


def cases():
    """(B, Lq, Lk, H, data): every (Lq, Lk) pair, H, B <= 3 and the data set cycling so that each value meets several partners;
    then the workflow shapes."""
    out = []
    for i, lk in enumerate(LK):
        for j, lq in enumerate(LQ):
            n = i * len(LQ) + j
            out.append((1 + n % 3, lq, lk, HEADS[(i + 2 * j) % 5], DATA_SETS[n % 4]))
    out += [(1, lq, 256, h, DATA_SETS[k % 4]) for k, (lq, h) in enumerate(WORKFLOW)]
    return out


def case_id(c):
    return "B{}-Lq{}-Lk{}-H{}-{}".format(*c)


def _bf(x, rnd):
    return x.to(torch.bfloat16).to(torch.float64) if rnd else x


def make_q_kv(B, Lq, Lk, H, data, salt=0):
    """Seeded (q [B, Lq, 64 H], kv [B, Lk, 128 H]) bf16: 'workflow' randn x 1.5; 'flat' q, k x 0.05 (near-uniform P: a dropped or
    doubled key and a wrong row sum move everything); 'sharp' q, k x 3; 'voff' workflow with V + 4."""
    g = torch.Generator().manual_seed(1000003 * B + 1009 * Lq + 31 * Lk + 17 * H + 7 * DATA_SETS.index(data) + salt)
    q = torch.randn(B, Lq, H * DH, generator=g)
    kv = torch.randn(B, Lk, 2, H * DH, generator=g)
    scale = {"flat": 0.05, "sharp": 3.0}.get(data, 1.5)
    q *= scale
    kv[:, :, 0] *= scale
    kv[:, :, 1] *= 1.5
    if data == "voff":
        kv[:, :, 1] += 4.0
    return q.to(torch.bfloat16), kv.reshape(B, Lk, 2 * H * DH).to(torch.bfloat16)


def attention_kv_f64(q, kv, H, rnd, fault=None):
    """[B, Lq, 64 H] float64: softmax(q k^T / 8) v per head.  ``rnd``: P rounded to bf16 (numerator and row sum alike) and the
    output rounded to bf16, as the kernel does.  ``fault``: one of FAULTS planted."""
    B, Lq, _ = q.shape
    Lk = kv.shape[1]
    qh = q.to(torch.float64).reshape(B, Lq, H, DH).permute(0, 2, 1, 3)
    k, v = kv.to(torch.float64).reshape(B, Lk, 2, H, DH).permute(2, 0, 3, 1, 4)
    if fault == "v_before_k":
        k, v = v, k
    if fault == "last_key_dropped":
        k, v = k[..., :-1, :], v[..., :-1, :]
    if fault == "last_key_doubled":
        k, v = torch.cat([k, k[..., -1:, :]], -2), torch.cat([v, v[..., -1:, :]], -2)
    if fault == "heads_rotated":
        k, v = torch.roll(k, 1, dims=1), torch.roll(v, 1, dims=1)          # a head reads the k | v of its neighbour
    s = qh @ k.transpose(-1, -2) / (np.sqrt(H * DH) if fault == "scale_1/sqrtC" else 8.0)
    p = _bf(torch.exp(s - s.amax(-1, keepdim=True)), rnd)
    o = (p @ v) / p.sum(-1, keepdim=True)
    return _bf(o.permute(0, 2, 1, 3).reshape(B, Lq, H * DH), rnd)


# fault -> the cases' property it needs
FAULTS = {"v_before_k": lambda c: True, "last_key_dropped": lambda c: c[2] >= 2, "last_key_doubled": lambda c: True,
          "heads_rotated": lambda c: c[3] >= 2, "scale_1/sqrtC": lambda c: c[3] >= 2 and c[2] >= 2}


def per_head(x, H):
    """[B, Lq, 64 H] -> numpy float64 [B H, Lq, 64]."""
    B, L, _ = x.shape
    return x.to(torch.float64).reshape(B, L, H, DH).permute(0, 2, 1, 3).reshape(B * H, L, DH).numpy()


def _worst(num, den):
    r = num / np.maximum(den, 1e-30)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max())


def head_err(got, ref):
    return _worst(np.sqrt(((got - ref) ** 2).sum((1, 2))), np.sqrt((ref ** 2).sum((1, 2))))


def row_err(got, ref):
    return _worst(np.sqrt(((got - ref) ** 2).sum(2)), np.sqrt((ref ** 2).sum(2)))


# ------------------------------------------------------------------------------------------------ the plan
def plan(B, Lq, Lk, H):
    """Mirror of att_kv_plan: dict(NT, NW, chunk, nchunks, grid, block, lds)."""
    if min(B, Lq, Lk, H) < 1 or Lk > 336:
        raise ValueError("outside the kernel's range")
    nt = -(-Lk // 16)
    NT = next(n for n in (6, 10, 17, 21) if nt <= n)
    NW = 8 if NT > 17 else 4
    BH, n_qt = B * H, -(-Lq // 16)
    slots = 512 if NW == 4 else 256                 # resident workgroups of a full machine
    per_head = -(-slots // BH)
    chunk = max(-(-n_qt // per_head), NW)           # never below one query tile per wave
    chunk = -(-chunk // NW) * NW
    nchunks = -(-n_qt // chunk)
    return dict(NT=NT, NW=NW, chunk=chunk, nchunks=nchunks, grid=BH * nchunks, block=64 * NW,
                lds=(NT * 16 + (NT + 1) // 2 * 32) * 128)
