"""Seeded cases of the frame warp (tests/test_frame_warp.py, tests/test_gpu_frame_warp.py, tests/golden/make_golden_frame_warp.py).

A case: source size, destination size, matrix (or one per frame), dtype, flags, border value, optional rectangle
(xmin, xmax, ymin, ymax) = destination rows and columns, and the number of frames.  ``case_inputs(name)`` rebuilds the frames.
"""
import zlib

import numpy as np

INTER_NEAREST, INTER_LINEAR, WARP_INVERSE_MAP = 0, 1, 16

YAML_ROI = (0, 720, 320, 960)     # hot_plate1.yaml's common_params: all 720 rows, columns 320 .. 960 of the 720 x 1280 sensor


def _rot_scale(deg, scale, cx, cy, tx=0.0, ty=0.0):
    a = np.deg2rad(deg)
    c, s = scale * np.cos(a), scale * np.sin(a)
    return np.array([[c, -s, cx - c * cx + s * cy + tx], [s, c, cy - s * cx - c * cy + ty], [0.0, 0.0, 1.0]])


# camera (1200 x 1920) -> event view (720 x 1280): scale, slight rotation, offset and mild perspective terms
HOMOGRAPHY = np.array([[0.6721, -0.0113, -18.37], [0.0094, 0.6689, -31.52], [2.1e-6, -1.3e-6, 1.0]])
SMALL_HOMOGRAPHY = np.array([[0.7412, -0.0131, -2.37], [0.0102, 0.6689, -1.52], [2.1e-5, -1.3e-5, 1.0]])    # 96 x 128 -> 64 x 96

CASES = {
    "identity_u8": dict(src=(40, 56), dst=(40, 56), M=np.eye(3), dtype="uint8"),
    "identity_f32": dict(src=(40, 56), dst=(40, 56), M=np.eye(3), dtype="float32"),
    "shift_int_u8": dict(src=(40, 56), dst=(40, 56), M=np.array([[1, 0, 3.0], [0, 1, -2.0], [0, 0, 1]]), dtype="uint8", border=7),
    "shift_32nds_u8": dict(src=(50, 70), dst=(48, 66), M=np.array([[1, 0, 13 / 32], [0, 1, -27 / 32], [0, 0, 1]]), dtype="uint8"),
    "shift_32nds_f32": dict(src=(50, 70), dst=(48, 66), M=np.array([[1, 0, 13 / 32], [0, 1, -27 / 32], [0, 0, 1]]), dtype="float32"),
    "rot_scale_u8": dict(src=(90, 130), dst=(75, 101), M=_rot_scale(17.0, 0.83, 60.0, 40.0, 2.25, -1.5), dtype="uint8", border=19),
    "rot_scale_f32": dict(src=(90, 130), dst=(75, 101), M=_rot_scale(17.0, 0.83, 60.0, 40.0, 2.25, -1.5), dtype="float32", border=-3.5),
    "rot_scale_nearest_u8": dict(src=(90, 130), dst=(75, 101), M=_rot_scale(-31.0, 1.21, 50.0, 45.0), dtype="uint8", flags=INTER_NEAREST),
    "rot_scale_nearest_f32": dict(src=(90, 130), dst=(75, 101), M=_rot_scale(-31.0, 1.21, 50.0, 45.0), dtype="float32",
                                  flags=INTER_NEAREST, border=0.25),
    "small_homography_u8": dict(src=(96, 128), dst=(64, 96), M=SMALL_HOMOGRAPHY, dtype="uint8", frames=3),
    "partly_outside_u8": dict(src=(60, 80), dst=(64, 100), M=_rot_scale(40.0, 1.6, 10.0, 70.0, 25.0, -12.0), dtype="uint8", border=200),
    "partly_outside_f32": dict(src=(60, 80), dst=(64, 100), M=_rot_scale(40.0, 1.6, 10.0, 70.0, 25.0, -12.0), dtype="float32", border=1.5),
    # an inverse map whose third row vanishes exactly on destination row 5 (W == 0 there) and changes sign across it
    "w_zero_line_u8": dict(src=(40, 56), dst=(24, 40), M=np.array([[1.0, 0.25, 2.0], [0.0, 1.5, 1.0], [0.0, 0.125, -0.625]]), dtype="uint8",
                           flags=INTER_LINEAR | WARP_INVERSE_MAP, border=33),
    "w_zero_line_nearest_f32": dict(src=(40, 56), dst=(24, 40), M=np.array([[1.0, 0.25, 2.0], [0.0, 1.5, 1.0], [0.0, 0.125, -0.625]]),
                                    dtype="float32", flags=INTER_NEAREST | WARP_INVERSE_MAP, border=-1.0),
    # 32 / W overflows to inf: column 0 is 0 * inf = NaN, the others inf -- all clamp to INT_MAX, outside the source
    "nan_coordinate_u8": dict(src=(40, 56), dst=(24, 40), M=np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1e-307]]), dtype="uint8",
                              flags=INTER_LINEAR | WARP_INVERSE_MAP, border=5),
    "nan_coordinate_f32": dict(src=(40, 56), dst=(24, 40), M=np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1e-307]]), dtype="float32",
                               flags=INTER_LINEAR | WARP_INVERSE_MAP, border=-2.5),
    "inverse_flag_u8": dict(src=(90, 130), dst=(75, 101), M=_rot_scale(9.0, 1.07, 33.0, 21.0, -4.125, 3.5), dtype="uint8",
                            flags=INTER_LINEAR | WARP_INVERSE_MAP),
    "per_frame_u8": dict(src=(70, 90), dst=(60, 84), frames=5, dtype="uint8", border=11,
                         M=np.stack([_rot_scale(4.0 * k - 7.0, 0.9 + 0.05 * k, 40.0, 30.0, 1.5 * k, -0.75 * k) for k in range(5)])),
    "per_frame_many_f32": dict(src=(30, 44), dst=(28, 36), frames=37, dtype="float32",     # more frames than one launch carries matrices for
                               M=np.stack([_rot_scale(2.0 * k - 30.0, 1.0 + 0.01 * k, 20.0, 15.0, 0.25 * k, 0.0) for k in range(37)])),
    "rect_u8": dict(src=(90, 130), dst=(75, 101), M=_rot_scale(17.0, 0.83, 60.0, 40.0, 2.25, -1.5), dtype="uint8", roi=(9, 61, 70, 99), frames=2),
    "rect_odd_f32": dict(src=(90, 130), dst=(75, 101), M=_rot_scale(17.0, 0.83, 60.0, 40.0, 2.25, -1.5), dtype="float32", roi=(40, 41, 33, 40)),
    "narrow_dst_u8": dict(src=(40, 56), dst=(9, 3), M=_rot_scale(5.0, 3.0, 1.0, 4.0), dtype="uint8"),      # H < 16, W < 4: block geometry, tail lanes
    "full_u8": dict(src=(1200, 1920), dst=(720, 1280), M=HOMOGRAPHY, dtype="uint8"),
    "full_roi_u8": dict(src=(1200, 1920), dst=(720, 1280), M=HOMOGRAPHY, dtype="uint8", roi=YAML_ROI, frames=2),
    "full_f32": dict(src=(1200, 1920), dst=(720, 1280), M=HOMOGRAPHY, dtype="float32"),
    "full_nearest_u8": dict(src=(1200, 1920), dst=(720, 1280), M=HOMOGRAPHY, dtype="uint8", flags=INTER_NEAREST),
}
SMALL = [n for n, c in CASES.items() if c["src"][0] < 1000]


def textured(rs, B, H, W, dtype):
    """Smooth structure plus noise: neighbouring pixels differ, so a one-pixel or one-fraction slip shows."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    frames = []
    for _ in range(B):
        a, b, c, d = rs.uniform(0.02, 0.3, 4)
        img = 110 + 60 * np.sin(a * xx + b * yy) + 40 * np.cos(c * xx - d * yy) + rs.uniform(-25, 25, (H, W))
        frames.append(img)
    f = np.stack(frames)
    if dtype == "uint8":
        return np.clip(np.rint(f), 0, 255).astype(np.uint8)
    return (f / 37.0 - 2.0).astype(np.float32)


def case_inputs(name):
    """-> (srcs [B, Hs, Ws], M [3, 3] | [B, 3, 3], dsize (W, H), flags, border_value, roi | None)."""
    c = CASES[name]
    rs = np.random.RandomState(zlib.crc32(name.encode()) % (2 ** 31))
    srcs = textured(rs, c.get("frames", 1), c["src"][0], c["src"][1], c["dtype"])
    return srcs, np.asarray(c["M"], dtype=np.float64), (c["dst"][1], c["dst"][0]), c.get("flags", INTER_LINEAR), c.get("border", 0), c.get("roi")
