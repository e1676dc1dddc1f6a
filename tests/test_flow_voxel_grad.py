"""CPU checks that pin tests/_flow_voxel_grad_ref.py, the yardstick of the GPU gradient tests, to gradients the reference's own
autograd produced (tests/golden/golden_flow_voxel_grad.npz, written by make_golden_flow_voxel_grad.py): every case of the fixture, in
float64 and float32, each against the reference's gradient of the same dtype within ``4 r_D max|reference gradient|``."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _flow_voxel_grad_ref as GR  # noqa: E402

G = GR.GOLDEN
STEPS = [(0.2, 1, 1), (-0.25, 2, 4), (1.0, 1, 1)]      # as in make_golden_flow_voxel_grad.py
DTS = [0.4, -0.7]
CLAMP = 1.5
DTYPES = {"t64": np.float64, "t32": np.float32}


def helper_gradient(case, dtype):
    kind, *rest = case.split("_")
    up = G["up_" + case]
    if kind == "vox":
        scheme, T, loc, c, key = rest
        flows = G["flow_" + key].astype(dtype)
        return GR.voxel_grad(flows, up, int(T), scheme, loc, CLAMP if c == "c" else None, torch_wrap=True)[1]
    if kind == "step":
        scheme, k, key = rest
        dt, dx, dy = STEPS[int(k)]
        return GR.step_grad(scheme, G["flow_" + key].astype(dtype), up, dt, dx, dy)[1]
    method, k, key = rest
    return GR.propagate_grad(G["flow_" + key][0].astype(dtype), up, DTS[int(k)], method)[1]


def test_the_fixture_measures_a_rounding_sized_r32_on_branch_stable_cases_of_every_scheme():
    cases, stable = [str(c) for c in G["cases"]], G["stable"]
    for scheme in ("upwind", "burgers", "same", "bilinear"):
        assert any(s and c.startswith("vox_" + scheme) for c, s in zip(cases, stable)), scheme
    assert 2.0 ** -24 < GR.R32 < 64 * 2.0 ** -24      # a few units of float32's roundoff: rounding, not a flipped branch


@pytest.mark.parametrize("tag", ["t64", "t32"])
def test_the_helper_gives_the_references_gradients(tag):
    dtype = DTYPES[tag]
    for case in (str(c) for c in G["cases"]):
        want = G[f"grad_{case}_{tag}"]
        got = helper_gradient(case, dtype)
        assert got.dtype == dtype and got.shape == want.shape, case
        err, tol = float(np.abs(got.astype(np.float64) - want).max()), GR.tolerance(dtype, want)
        assert err <= tol, f"{case} {tag}: |helper - reference| = {err:.3e} > {tol:.3e}"


def test_the_tie_rule_is_half_and_half():
    """The flow with one non-zero pixel: maximum(x, 0) and minimum(x, 0) hand half the gradient each to an exact zero, which a
    one-sided rule does not reproduce.  One upwind step with dt = 1 and an upstream gradient of ones: the pixel below the non-zero one
    gets 1 - dt * (d_max0 * u_dx_back + d_min0 * u_dx_forw) = 1 - (0.5 * (0 - 1) + 0.5 * 0) = 1.5 (one-sided: 1 or 2)."""
    flow = np.zeros((1, 2, 5, 5))
    flow[0, 0, 2, 2] = 1.0
    _, g = GR.step_grad("upwind", flow, np.ones_like(flow), 1.0)
    assert g[0, 0, 3, 2] == 1.5
