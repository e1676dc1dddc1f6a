"""CPU tests of the contrast's Hessian-vector product: the closed form the kernels implement against torch's float64 double backward,
the argument checks of the two C entries (before any launch), the solver's acceptance of the second-order scipy methods and the
refusals of the plan operators.  Cases and yardsticks: tests/_hvp_cases.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hvp_cases as C  # noqa: E402
from _hvp_cases import H, W, rel  # noqa: E402

HESSP_METHODS = ("Newton-CG", "trust-ncg", "trust-krylov")


@pytest.fixture(scope="module")
def lib():
    from event_based_bos_amd import _hip
    from event_based_bos_amd.build import build_library

    build_library(verbose=False)
    return _hip.load_library()


# ---------------------------------------------------------------------------------------------- the formula
@pytest.mark.parametrize("blur", [0.0, 1.0])
@pytest.mark.parametrize("pad", [0, 2])
@pytest.mark.parametrize("omit", [False, True])
@pytest.mark.parametrize("cost", ["image_variance", "gradient_magnitude"])
def test_closed_form_is_float64_autograd(cost, omit, pad, blur):
    """value, gradient and product of the closed form (float64) against ``torch.autograd.functional.hvp`` of the float64 expression."""
    ev, flow, v = C.kink_free(), C.flow_u(), C.direction_v()
    value, grad, hv = C.ref_hvp("kf", ev, flow, v, cost, omit, pad, blur)
    got_value, got_grad, got_hv, _, _ = C.closed_form(ev, flow, v, cost, omit, pad, blur)
    errs = (abs(got_value - value) / abs(value), rel(got_grad, grad), rel(got_hv, hv))
    print(f"{cost} omit={omit} pad={pad} blur={blur}: value rel {errs[0]:.2e}, d_flow rel L2 {errs[1]:.2e}, hv rel L2 {errs[2]:.2e}")
    assert np.linalg.norm(hv) > 0 and max(errs) < 1e-12


def test_closed_form_images_and_the_weight_of_the_cross_term():
    """The tangent image is autograd's directional derivative of the IWE; and the curvature of the bilinear weights (``cross``) is no
    small part of the product: an implementation that drops it (Gauss-Newton) is far outside every bar of the GPU tests."""
    ev, flow, v = C.kink_free(), C.flow_u(), C.direction_v()
    iwe, tangent = C.ref_images("kf", ev, flow, v, 0)
    _, _, hv, got_iwe, got_tangent = C.closed_form(ev, flow, v)
    assert rel(got_iwe, iwe) < 1e-12 and rel(got_tangent, tangent) < 1e-12
    # the Gauss-Newton part alone: J^T (grad cost at the tangent image), by autograd through the IWE
    f = torch.from_numpy(flow).clone().requires_grad_(True)
    img = C.O.iwe_dense(torch.from_numpy(ev), f, (H, W), (0, 0), "first", True)
    g2 = C._grad_map(torch.from_numpy(got_tangent), "image_variance", False, 0.0)[1]
    (gauss_newton,) = torch.autograd.grad((img * g2).sum(), f)
    share = np.linalg.norm(hv - gauss_newton.numpy()) / np.linalg.norm(hv)
    print(f"the cross term carries {share:.1%} of |Hv|")
    assert share > 0.2


def test_closed_form_in_float32_is_close():
    """The same formula evaluated in float32 on the CPU: the size of the rounding the float32 kernels may show."""
    ev, flow, v = C.kink_free(), C.flow_u(), C.direction_v()
    _, grad, hv = C.ref_hvp("kf", ev, flow, v)
    _, got_grad, got_hv, _, _ = C.closed_form(ev, flow, v, dtype=torch.float32)
    print(f"float32 closed form: d_flow rel L2 {rel(got_grad, grad):.2e}, hv rel L2 {rel(got_hv, hv):.2e}")
    assert rel(got_hv, hv) < 1e-3 and rel(got_grad, grad) < 1e-3


# ---------------------------------------------------------------------------------------------- the C entries
P = 0x1000   # a pointer that is never read: only calls that are refused before any launch get it


def _tangent_args(**over):
    a = dict(xs=P, ys=P, dts=P, key_offsets=P, n=10, flow=P, v=P, H=37, W=70, tile_h=32, tile_w=32, halo=8, splits=1, pad_h=0, pad_w=0,
             iwe=P, tangent=P, stream=None)
    a.update(over)
    return list(a.values())


def _owner_args(**over):
    a = dict(xs=P, ys=P, dts=P, key_offsets=P, n=10, flow=P, v=P, H=37, W=70, tile_h=32, tile_w=32, pad_h=0, pad_w=0, g1=P, g2=P,
             affine=None, g_lo=0, d_flow=None, hv=P, stream=None)
    a.update(over)
    return list(a.values())


def test_entries_refuse_before_any_launch(lib):
    """NULL buffers and bad sizes: -1 with a message; a (tile, halo) that is not built or does not fit the LDS: -3
    (EBOS_ERR_UNSUPPORTED) -- all before the first HIP call, so this runs without a GPU."""
    tangent, owner = lib.ebos_iwe_dense_tangent_tiled_f32, lib.ebos_iwe_dense_hvp_owner_bwd_f32
    for over, text in ((dict(flow=None), b"NULL flow/v/tangent"), (dict(v=None), b"NULL flow/v/tangent"),
                       (dict(tangent=None), b"NULL flow/v/tangent"), (dict(key_offsets=None), b"key_offsets is NULL"),
                       (dict(xs=None), b"NULL event buffer"), (dict(splits=0), b"bad sizes"), (dict(H=0), b"bad sizes"),
                       (dict(n=-1), b"bad sizes"), (dict(pad_h=-1), b"bad sizes")):
        assert tangent(*_tangent_args(**over)) == -1, over
        assert lib.ebos_last_error().startswith(b"ebos_iwe_dense_tangent_tiled: ") and text in lib.ebos_last_error(), over
    for over in (dict(tile_h=33), dict(halo=7), dict(tile_h=64, tile_w=64, halo=64),          # not built; built, two windows too many
                 dict(tile_h=45, tile_w=80, halo=32)):                                        # a slab tile without a tiled kernel
        assert tangent(*_tangent_args(**over)) == -3, over
        assert lib.ebos_last_error().startswith(b"ebos_iwe_dense_tangent_tiled: "), over
    assert lib.ebos_iwe_multiref_fits(64, 64, 64, 1) == 1 and lib.ebos_iwe_multiref_fits(64, 64, 64, 2) == 0
    assert tangent(*_tangent_args(n=0, xs=None, ys=None, dts=None)) == 0                      # nothing to launch
    # the slab form: the same checks under its own name, a workspace of ebos_iwe_tangent_slab_workspace_bytes
    slab, need = lib.ebos_iwe_dense_tangent_slab_f32, lib.ebos_iwe_tangent_slab_workspace_bytes
    assert need(37, 70, 32, 32, 8, 2) == 6 * 2 * 48 * 48 * 8 and need(37, 70, 32, 32, 8, 1) == 6 * 48 * 48 * 8       # f64 windows
    assert need(720, 1280, 64, 64, 32, 2) == 12 * 20 * 2 * 128 * 128 * 4                                              # f32 windows
    assert need(37, 70, 33, 32, 8, 2) == 0 and need(37, 70, 64, 64, 64, 2) == 0 and need(37, 70, 32, 32, 8, 3) == 0 and need(0, 70, 32, 32, 8, 1) == 0

    def slab_args(**over):
        a = dict(xs=P, ys=P, dts=P, key_offsets=P, n=10, flow=P, v=P, H=37, W=70, tile_h=32, tile_w=32, halo=8, pad_h=0, pad_w=0,
                 workspace=P, workspace_bytes=need(37, 70, 32, 32, 8, 2), iwe=P, tangent=P, stream=None)
        a.update(over)
        return list(a.values())

    for over, rc, text in ((dict(v=None), -1, b"NULL flow/v/tangent"), (dict(key_offsets=None), -1, b"key_offsets is NULL"),
                           (dict(W=0), -1, b"bad sizes"), (dict(workspace=None), -1, b"workspace is NULL"),
                           (dict(workspace_bytes=need(37, 70, 32, 32, 8, 2) - 1), -4, b"workspace too small"),
                           (dict(tile_h=64, tile_w=64, halo=64), -3, b"do not fit the LDS")):
        assert slab(*slab_args(**over)) == rc, over
        assert lib.ebos_last_error().startswith(b"ebos_iwe_dense_tangent_slab: ") and text in lib.ebos_last_error(), over
    assert slab(*slab_args(n=0, xs=None, ys=None, dts=None)) == 0
    for over, text in ((dict(flow=None), b"NULL flow/v/g1/g2/hv"), (dict(v=None), b"NULL flow/v/g1/g2/hv"),
                       (dict(g1=None), b"NULL flow/v/g1/g2/hv"), (dict(g2=None), b"NULL flow/v/g1/g2/hv"),
                       (dict(hv=None), b"NULL flow/v/g1/g2/hv"), (dict(key_offsets=None), b"key_offsets is NULL"),
                       (dict(ys=None), b"NULL event buffer"), (dict(g_lo=-1), b"bad sizes"), (dict(tile_w=0), b"bad sizes")):
        assert owner(*_owner_args(**over)) == -1, over
        assert lib.ebos_last_error().startswith(b"ebos_iwe_dense_hvp_owner_bwd: ") and text in lib.ebos_last_error(), over


def test_entries_are_declared_built_and_mirrored():
    from event_based_bos_amd import _hip
    from event_based_bos_amd.build import SOURCES

    assert "iwe_hvp.hip" in SOURCES and _hip.ABI_VERSION == 2
    assert len(_hip.SIGNATURES["ebos_iwe_dense_tangent_tiled_f32"][1]) == 18
    assert len(_hip.SIGNATURES["ebos_iwe_dense_hvp_owner_bwd_f32"][1]) == 20
    assert len(_hip.SIGNATURES["ebos_iwe_dense_tangent_slab_f32"][1]) == 19


# ---------------------------------------------------------------------------------------------- solver construction
def _solver(cfg):
    from event_based_bos_amd.solver.contrast_maximization import ContrastMaximization

    return ContrastMaximization((H, W), (H, W), solver_config=cfg)


@pytest.mark.parametrize("method", HESSP_METHODS)
def test_solver_accepts_the_methods_on_dense_flow(method):
    from event_based_bos_amd.solver import contrast_maximization as CM

    assert CM.SCIPY_HESSP_METHODS == HESSP_METHODS and not set(HESSP_METHODS) & set(CM.SCIPY_METHODS)
    slv = _solver(C.solver_config(method, tile=None))
    assert slv.hessp and slv.hessp_calls == 0 and not slv.fused_loop and not slv.use_graph and slv.resident is False
    assert tuple(slv.plan_tile()) == CM.MULTI_REFERENCE_TILE                          # without an explicit tile
    assert tuple(_solver(C.solver_config(method)).plan_tile()) == C.TILE
    assert not _solver(C.solver_config("L-BFGS-B")).hessp and not _solver(C.solver_config("Adam")).hessp


@pytest.mark.parametrize("method", HESSP_METHODS)
@pytest.mark.parametrize("case", ["2d-translation", "rigid-optical-flow", "time_aware", "time_aware-native", "time_aware-directions",
                                  "multi_reference", "multi_reference-native"])
def test_solver_refuses_the_methods_elsewhere(case, method):
    """Outside the plain dense-flow warp the three names stay what every unknown method is: NotImplementedError, naming the key."""
    over = {}
    if case in ("2d-translation", "rigid-optical-flow"):
        over["motion_model"] = case
    elif case.startswith("time_aware"):
        over["time_aware"] = {"time_bin": 4}
        if case.endswith("native"):
            over["time_aware"]["native"] = True
        if case.endswith("directions"):
            over["time_aware"]["directions"] = ["first", "last"]
    else:
        over["multi_reference"] = {"directions": ["first", "last"]}
        if case.endswith("native"):
            over["multi_reference"]["native"] = True
    with pytest.raises(NotImplementedError, match="optimizer.method"):
        _solver(C.solver_config(method, tile=(64, 64), **over))


# ---------------------------------------------------------------------------------------------- plan operators
def _host_plan(**over):
    """A binned full plan of three events in host memory: the refusals under test come before anything touches the GPU."""
    from event_based_bos_amd.event_plan import EventPlan

    z = torch.zeros(3, dtype=torch.float32)
    keys = (H + 31) // 32 * ((W + 31) // 32) * 32 * 32
    kw = dict(x=z, y=z, dt=z, p=z, image_size=(H, W), n=3, n_input=3, tile=(32, 32), key_offsets=torch.zeros(keys + 1, dtype=torch.int32))
    kw.update(over)
    return EventPlan(**kw)


@pytest.mark.parametrize("op", ["contrast_dense_hvp", "iwe_dense_jvp"])
def test_plan_operators_refuse(op):
    flow = torch.zeros((2, H, W), dtype=torch.float32)
    lean = _host_plan(x=None, y=None, dt=None, p=None)
    deferred = _host_plan()
    deferred.__dict__["_deferred"] = True
    for plan, text in ((lean, "lean plan"), (deferred, "deferred=True"), (_host_plan(tile=None, key_offsets=None), "binned plan"),
                       (_host_plan(tile=(45, 80)), r"no built halo of tile \(45, 80\)")):
        with pytest.raises(NotImplementedError, match=text):
            getattr(plan, op)(flow, flow)
    with pytest.raises(NotImplementedError, match="per-event weights"):
        getattr(_host_plan(), op)(flow, flow, weight=torch.ones(3))
    for bad_flow, bad_v in ((flow[:, :-1], flow), (flow, flow[:1]), (flow.to(torch.int32), flow), (flow, flow.to(torch.int64))):
        with pytest.raises(ValueError):
            getattr(_host_plan(), op)(bad_flow, bad_v)
    if op == "contrast_dense_hvp":
        with pytest.raises(KeyError):
            _host_plan().contrast_dense_hvp(flow, flow, cost="sharpness")
        with pytest.raises(KeyError):
            _host_plan().contrast_dense_hvp(flow, flow, cost={"image_variance": 1.0, "sharpness": 1.0})


# ---------------------------------------------------------------------------------------------- every built triple (host side)
# (tile_h, tile_w, halo) -> (ebos_iwe_multiref_fits with 1 window, with 2): 2 = float64 windows, 1 = float32, 0 = they do not fit
FITS_TABLE = {(64, 64, 32): (2, 1), (32, 64, 32): (2, 1), (32, 32, 32): (2, 2), (16, 64, 32): (2, 2), (64, 64, 16): (2, 2),
              (32, 32, 16): (2, 2), (32, 32, 8): (2, 2), (64, 64, 64): (1, 0), (32, 64, 48): (2, 1)}
# ... and the dynamic LDS of the launch, windows * (tile_h + 2 halo) * (tile_w + 2 halo) * sizeof(accumulator)
LDS_TABLE = {(64, 64, 32): (131072, 131072), (32, 64, 32): (98304, 98304), (32, 32, 32): (73728, 147456), (16, 64, 32): (81920, 163840),
             (64, 64, 16): (73728, 147456), (32, 32, 16): (32768, 65536), (32, 32, 8): (18432, 36864), (64, 64, 64): (147456, None),
             (32, 64, 48): (163840, 163840)}


def test_fits_table_of_every_built_triple(lib):
    """Which accumulator the tangent kernel (and the multi-reference kernel, with K = windows) runs with per built triple, and the
    LDS it asks for: three launches take the whole 160 KiB."""
    from event_based_bos_amd import _hip

    assert set(_hip.tiled_configs()) == set(FITS_TABLE)
    at_limit = []
    for (th, tw, hl), kinds in FITS_TABLE.items():
        for windows, kind, lds in zip((1, 2), kinds, LDS_TABLE[(th, tw, hl)]):
            assert lib.ebos_iwe_multiref_fits(th, tw, hl, windows) == kind, (th, tw, hl, windows)
            if kind:
                assert windows * (th + 2 * hl) * (tw + 2 * hl) * (8 if kind == 2 else 4) == lds <= 160 * 1024
                at_limit += [((th, tw, hl), windows, kind)] if lds == 160 * 1024 else []
            else:
                assert lds is None and windows * (th + 2 * hl) * (tw + 2 * hl) * 4 > 160 * 1024
    assert at_limit == [((16, 64, 32), 2, 2), ((32, 64, 48), 1, 2), ((32, 64, 48), 2, 1)]
    # the multi-reference forms of the same limits: K windows
    assert lib.ebos_iwe_multiref_fits(16, 64, 32, 4) == 1 and lib.ebos_iwe_multiref_fits(32, 64, 48, 3) == 0


@pytest.mark.parametrize("shape", [(70, 135), (13, 21)])
def test_tangent_slab_workspace_is_tiles_times_windows(lib, shape):
    """``ebos_iwe_tangent_slab_workspace_bytes`` = tiles * windows * LH * LW * sizeof(accumulator), the accumulator that of the table."""
    H_, W_ = shape
    for (th, tw, hl), kinds in FITS_TABLE.items():
        tiles = -(-H_ // th) * -(-W_ // tw)
        for windows, kind in zip((1, 2), kinds):
            want = tiles * windows * (th + 2 * hl) * (tw + 2 * hl) * {2: 8, 1: 4, 0: 0}[kind]
            assert lib.ebos_iwe_tangent_slab_workspace_bytes(H_, W_, th, tw, hl, windows) == want, (shape, th, tw, hl, windows)
    assert lib.ebos_iwe_tangent_slab_workspace_bytes(70, 135, 64, 64, 16, 2) == 6 * 2 * 96 * 96 * 8
    assert lib.ebos_iwe_tangent_slab_workspace_bytes(13, 21, 32, 64, 48, 2) == 1 * 2 * 128 * 160 * 4


def test_hvp_halo_choices_per_tile(lib):
    """``_hvp_halo`` with "auto": the largest built halo of the tile whose windows are float64, failing that float32 -- with the IWE
    (2 windows) / without (1); an explicit halo that fits is honoured, float32 windows included; one that does not falls back."""
    from event_based_bos_amd import event_plan as EP

    for tile, (two, one) in {(64, 64): (16, 32), (32, 64): (48, 48), (32, 32): (32, 32), (16, 64): (32, 32)}.items():
        plan = _host_plan(tile=tile)
        assert (EP._hvp_halo(plan, "auto", 2, "test"), EP._hvp_halo(plan, "auto", 1, "test")) == (two, one), tile
        assert EP._hvp_halo(plan, None, 2, "test") == two
    for windows in (1, 2):
        with pytest.raises(NotImplementedError, match=r"no built halo of tile \(45, 80\)"):
            EP._hvp_halo(_host_plan(tile=(45, 80)), "auto", windows, "test")
    big = _host_plan(tile=(64, 64))
    assert EP._hvp_halo(big, 32, 2, "test") == 32 and lib.ebos_iwe_multiref_fits(64, 64, 32, 2) == 1       # honoured as float32
    assert EP._hvp_halo(big, 64, 1, "test") == 64 and EP._hvp_halo(big, 16, 1, "test") == 16
    assert EP._hvp_halo(big, 64, 2, "test") == 16                                                           # does not fit: falls back
    assert EP._hvp_halo(_host_plan(tile=(32, 64)), 32, 2, "test") == 32 and EP._hvp_halo(_host_plan(tile=(32, 32)), 8, 2, "test") == 8


def test_per_cell_bars_hold_ten_times_over_in_float32():
    """tests/test_gpu_hvp_tiles.py asserts every bar per cell as well, max |got - want| <= bar * max |want|.  What float32 arithmetic
    alone does to that form -- the closed form in float32 on the CPU against the float64 yardstick, 70 x 135, 30 000 events -- must
    sit at least ten times inside the bars (observed: IWE 2.4e-6, tangent 2.6e-6, d_flow 6.2e-6, hv 3.4e-6)."""
    import _hvp_tile_cases as T

    dev = T.float32_cpu_deviation()
    print("float32 closed form, per cell: " + ", ".join(f"{k} {v:.2e}" for k, v in dev.items()))
    assert max(dev["iwe"], dev["tangent"]) < 1e-5 and max(dev["d_flow"], dev["hv"]) < 1e-4


@pytest.mark.parametrize("method", HESSP_METHODS)
def test_solver_refuses_a_tile_with_float32_windows(lib, method):
    """The second-order methods need bits that repeat: a (tile, halo) whose two windows fit the LDS as float32 only is refused at
    construction, with the tiles that work (tests/test_gpu_hvp_tiles.py::test_solver_on_a_tile_with_float32_windows: what was
    measured).  No GPU is needed to say so."""
    from event_based_bos_amd import event_plan as EP

    assert EP.hvp_float64_tiles() == [(16, 64), (32, 32), (64, 64)]
    with pytest.raises(NotImplementedError, match=r"tile \[32, 64\].*float32.*\[16, 64\], \[32, 32\], \[64, 64\]"):
        _solver(C.solver_config(method, tile=(32, 64)))
    with pytest.raises(NotImplementedError, match=r"tile \[64, 64\], halo 32.*float32"):
        _solver(C.solver_config(method, tile=(64, 64), halo=32))
    with pytest.raises(NotImplementedError, match=r"no built halo of tile \(45, 80\)"):
        _solver(C.solver_config(method, tile=(45, 80)))
    for tile, halo in (((16, 64), "auto"), ((32, 32), 8), ((64, 64), 16), ((64, 64), 64)):    # (halo 64: two windows fall back to 16)
        assert _solver(C.solver_config(method, tile=tile, halo=halo)).hessp
    assert not _solver(C.solver_config("L-BFGS-B", tile=(32, 64))).hessp                      # the first-order methods take any tile
