"""CNF.decode_write_scales on the host (a stub network and torch CPU state arithmetic): under an error-controlled solver every
scale gets its own steps, as in the reference's sweep of one solve per scale (tools/utils_vis.py:189-198); under a fixed-step
solver the sweep stays one batched solve."""
import pytest
import torch

from tests.test_host_logic import TorchCpuOps


class _ScaledNet(torch.nn.Module):
    """v = -x + write_scale * sin(8 t) * x: the step sizes an error-controlled solve picks depend on the scale."""

    def __init__(self):
        super().__init__()
        self.rows = []

    def forward(self, x, t, *args, write_scale=0.0, **kwargs):
        self.rows.append(x.shape[0])
        ws = write_scale.view(-1, 1, 1, 1) if torch.is_tensor(write_scale) else float(write_scale)
        return -x + ws * torch.sin(8.0 * t.reshape(-1)[0]) * x, None


def _cnf():
    from uspace_amd.flow_matching import CNF
    cnf = CNF(_ScaledNet())
    cnf.state_ops_factory = TorchCpuOps
    return cnf


SK = dict(solver_fix="euler", solver_fix_step=0.05, solver_adaptive="dopri5", solver_adaptive_prec=0.01)
SCALES = [-3.0, 0.0, 0.5, 4.0]


@pytest.mark.parametrize("solver", ["fixadp", "adaptive"])
def test_error_controlled_sweep_equals_the_sequential_solves(solver):
    cnf = _cnf()
    z = torch.randn(2, 4, 4, 4, generator=torch.Generator().manual_seed(3))
    kw = dict(dissect_name="write_attr", t_edit=0.4, solver_kwargs=dict(SK, solver=solver))
    seq, nfe = [], 0
    for s in SCALES:
        seq.append(cnf.decode(z, None, write_scale=s, **kw))
        nfe += cnf.last_stats.nfe
    cnf.net.rows.clear()
    bat = cnf.decode_write_scales(z, None, SCALES, **kw)
    torch.testing.assert_close(bat, torch.stack(seq), rtol=1e-6, atol=1e-6)
    n_fixed = 8 if solver == "fixadp" else 0                       # Euler 0.05 up to 0.4, shared by every scale
    assert cnf.last_stats.nfe == nfe - (len(SCALES) - 1) * n_fixed
    assert cnf.net.rows[:n_fixed] == [len(SCALES) * 2] * n_fixed and set(cnf.net.rows[n_fixed:]) == {2}
    # one shared solve over all rows (the previous behaviour) takes other steps: the split is what makes the sweep exact
    rows = torch.tensor(SCALES).repeat_interleave(2)
    shared = cnf.decode(z.repeat(len(SCALES), 1, 1, 1), None, write_scale=rows, **kw).view_as(bat)
    assert (shared - bat).abs().max() > 1e-6


def test_fixed_step_sweep_stays_one_batched_solve():
    cnf = _cnf()
    z = torch.randn(2, 4, 4, 4, generator=torch.Generator().manual_seed(3))
    kw = dict(dissect_name="write_attr", t_edit=0.4, solver_kwargs=dict(SK, solver="fixed"))
    bat = cnf.decode_write_scales(z, None, SCALES, **kw)
    assert cnf.last_stats.nfe == 20 and set(cnf.net.rows) == {len(SCALES) * 2}
    seq = torch.stack([cnf.decode(z, None, write_scale=s, **kw) for s in SCALES])
    torch.testing.assert_close(bat, seq, rtol=1e-6, atol=1e-6)
