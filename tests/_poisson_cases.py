"""Inputs of the Poisson-integration fixture (tests/golden/golden_poisson.npz), regenerated from seeds.

Every case is a flow [2, H, W] of smooth displacement bumps plus noise and a boundary image (zeros, as every reference caller
passes, or random).  ``case_inputs(name)`` rebuilds (flow, boundary) exactly as tests/golden/make_golden_poisson.py handed them to
the reference -- as ``poisson_reconstruct(flow[1], flow[0], boundary)``, the component views the visualizer passes.

The fixture keeps the reference's float64 / float32 values bit for bit.  For cases larger than 64 x 64 it keeps them on the rows
``stored_rows(name)`` only (every 8th row plus the last two; float64 noise does not compress, and a full 260 x 346 field is 700 KB),
together with the whole uint8 picture and max|P| of the whole field; ``golden_case`` returns those.
"""
import numpy as np

# name -> (H, W, flow dtype, boundary dtype, boundary kind, seed)
CASES = {
    "s3x3_f64_zero": (3, 3, np.float64, np.float64, "zero", 1),
    "s3x3_f32_rand": (3, 3, np.float32, np.float32, "rand", 2),
    "s4x5_f64_rand": (4, 5, np.float64, np.float64, "rand", 3),
    "s4x5_f32_zero": (4, 5, np.float32, np.float32, "zero", 4),
    "s31x47_f64_zero": (31, 47, np.float64, np.float64, "zero", 5),
    "s31x47_f64_rand": (31, 47, np.float64, np.float64, "rand", 6),
    "s31x47_f32_zero": (31, 47, np.float32, np.float32, "zero", 7),
    "s31x47_f32_rand": (31, 47, np.float32, np.float32, "rand", 8),
    "s64x64_f64_rand": (64, 64, np.float64, np.float64, "rand", 9),
    "s64x64_f32_zero": (64, 64, np.float32, np.float32, "zero", 10),
    "s64x64_f32in_f64out_rand": (64, 64, np.float32, np.float64, "rand", 11),
    "s260x346_f64_zero": (260, 346, np.float64, np.float64, "zero", 12),
    "s260x346_f32_rand": (260, 346, np.float32, np.float32, "rand", 13),
}


def synth_flow(H, W, seed, dtype=np.float64, bumps=4, amplitude=3.0, noise=0.05):
    """[2, H, W]: a few Gaussian displacement bumps per component plus white noise."""
    rs = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    flow = np.zeros((2, H, W))
    for c in range(2):
        for _ in range(bumps):
            cy, cx = rs.uniform(0, H), rs.uniform(0, W)
            s = rs.uniform(0.1, 0.4) * max(H, W)
            flow[c] += rs.uniform(-amplitude, amplitude) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
    flow += rs.normal(0.0, noise, flow.shape)
    return flow.astype(dtype)


def case_inputs(name):
    """(flow [2, H, W], boundary [H, W]) of a case."""
    H, W, fdt, bdt, kind, seed = CASES[name]
    flow = synth_flow(H, W, seed, fdt)
    if kind == "zero":
        boundary = np.zeros((H, W), dtype=bdt)
    else:
        boundary = np.random.RandomState(seed + 1000).uniform(-2.0, 2.0, (H, W)).astype(bdt)
    return flow, boundary


ROW_STEP = 8          # cases larger than FULL_PIXELS keep every ROW_STEP-th row of the reference's field (and the last two)
FULL_PIXELS = 64 * 64


def stored_rows(name):
    """The rows of the reference's field the fixture keeps: None = all of them."""
    H, W = CASES[name][:2]
    if H * W <= FULL_PIXELS:
        return None
    return np.unique(np.r_[np.arange(0, H, ROW_STEP), H - 2, H - 1])


def golden_case(golden, name):
    """(rows, P_rows, u8, absmax): the rows of the field the fixture holds (a slice or an index array), the reference's values on
    them (its dtype), its whole uint8 picture and max|P| over the whole field (as float64)."""
    rows = stored_rows(name)
    return (slice(None) if rows is None else rows, golden[name + "_P"], golden[name + "_u8"], float(golden[name + "_absmax"]))
