import numpy as np
import torch


def rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def fault_projection(got, ref, bad, true):
    """How much of a planted fault the result carries: c_f = <got - ref, d_f> / <d_f, d_f> with the fault's direction
    d_f = bad - true (the faulty and the true float64 model from the same input).  0 for a correct kernel, 1 for one with the
    fault; rounding noise is spread over every element and nearly orthogonal to d_f.  ``ref`` is the model that rounds where the
    kernel rounds, so that got - ref is noise alone; torch tensors, evaluated in float64."""
    r = (got.double() - ref.double()).reshape(-1)
    d = (bad.double() - true.double()).reshape(-1)
    return float(torch.dot(r, d) / torch.dot(d, d))


def bf16_round(a):
    """fp32 numpy -> values representable in bf16 (RNE), still fp32."""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def to_dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype=dtype)


def load_sd(golden_dir, name):
    import os
    z = np.load(os.path.join(golden_dir, name))
    return z, {k[3:]: z[k] for k in z.files if k.startswith("sd/")}
