#!/usr/bin/env python3
"""Generate tests/golden/golden_frame_warp.npz by running the REFERENCE's co-capture loader, ``CcsDataLoader``
(src/data_loader/ccs.py: ``set_image_cache`` :136-156, ``load_frame_timestamps`` :36-47, ``image_index_to_time`` :332-343,
``time_to_image_index`` :359-371, ``load_image`` :373-396) on a tiny synthetic sequence written to a temporary directory.  Runs
only where the reference is checked out (see make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_frame_warp.py

OpenCV is absent here: ``cv2.imread`` is PIL and ``cv2.warpPerspective`` is the numpy restatement of tests/_warp_ref.py, and the
fixture carries ``shimmed = 1``.  So the fixture pins what the reference's wrapper does around the warp -- the (width, height)
order of ``dsize``, ``np.loadtxt`` of the homography, the positive-edge filter of both trigger formats, the division by 1e6, the
index arithmetic, the sorted suffix-filtered file list -- and, for the warp itself, only the restatement; OpenCV's own bits are
not pinned.
"""
import os
import shutil
import sys
import tempfile
import types
import warnings

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import import_reference  # noqa: E402
import _warp_ref as R  # noqa: E402
from _warp_cases import SMALL_HOMOGRAPHY, textured  # noqa: E402

SENSOR = (64, 96)        # (height, width) of the event view
CAMERA = (96, 128)
N_FRAMES = 6


def install_cv2_shim(calls):
    cv2 = types.ModuleType("cv2")
    cv2.IMREAD_GRAYSCALE = 0

    def imread(path, flags=None):
        assert flags == cv2.IMREAD_GRAYSCALE
        with Image.open(path) as im:
            return np.asarray(im.convert("L"), dtype=np.uint8)

    def warpPerspective(src, M, dsize, *args, **kwargs):
        assert not args and not kwargs                      # (the reference passes nothing else: INTER_LINEAR, constant 0 border)
        calls.append((np.array(M), tuple(dsize)))
        return R.warp_perspective(src, M, dsize)

    cv2.imread, cv2.warpPerspective = imread, warpPerspective
    sys.modules["cv2"] = cv2
    return cv2


def trigger_rows(rs, n):
    """A positive and a negative edge per frame (microseconds), plus a stray negative edge first."""
    t = 1_000_000 + np.cumsum(rs.randint(3000, 9000, n))
    rows = [(int(t[0]) - 700, 0, 0)]
    for v in t:
        rows += [(int(v), 0, 1), (int(v) + 1500, 0, 0)]
    return rows


def main():
    import_reference()
    calls = []
    cv2 = install_cv2_shim(calls)
    import src.data_loader.ccs as ccs
    from src.data_loader.base import DataLoaderBase

    ccs.cv2 = cv2
    rs = np.random.RandomState(20240611)
    frames = textured(rs, N_FRAMES, CAMERA[0], CAMERA[1], "uint8")
    rows = trigger_rows(rs, N_FRAMES)
    text = {"old": "".join(f"{t} {i} {p}\n" for t, i, p in rows), "new": "".join(f"{p},{i},{t}\n" for t, i, p in rows)}
    hom_text = "\n".join(" ".join(repr(float(v)) for v in row) for row in SMALL_HOMOGRAPHY) + "\n"
    out = {"shimmed": np.array(1), "frames": frames, "sensor_size": np.array(SENSOR), "homography_text": np.array(hom_text),
           "trigger_text_old": np.array(text["old"]), "trigger_text_new": np.array(text["new"])}
    root = tempfile.mkdtemp()
    try:
        seq = os.path.join(root, "CCS", "seq0")
        frame_dir = os.path.join(seq, "basler_0", "frames")
        os.makedirs(frame_dir)
        os.makedirs(os.path.join(seq, "prophesee_0"))
        for k in range(N_FRAMES):
            Image.fromarray(frames[k]).save(os.path.join(frame_dir, f"frame_{k:05d}.png"))
        with open(os.path.join(frame_dir, "frames.csv"), "w") as f:       # not an image suffix: the loader skips it
            f.write("index\n")
        with open(os.path.join(seq, "homography.txt"), "w") as f:
            f.write(hom_text)
        load_indices = [0, 3, N_FRAMES - 1]
        for fmt in ("old", "new"):
            with open(os.path.join(seq, "prophesee_0", "trigger_events.txt"), "w") as f:
                f.write(text[fmt])
            for warp in (True, False):
                loader = ccs.CcsDataLoader({"height": SENSOR[0], "width": SENSOR[1], "root": root, "dataset": "CCS", "warp": warp})
                DataLoaderBase.set_sequence(loader, "seq0")       # (the file names only: the event half needs h5py and a recording)
                assert loader.num_images == N_FRAMES
                if warp:
                    out["num_images"] = np.array(loader.num_images)
                    out["timestamps_" + fmt] = np.array(loader._image_cache["timestamp"])
                    out["homography"] = np.array(loader._image_cache["homography"])
                    idx = np.array([0, 1, N_FRAMES - 1, -1])
                    out["image_index_to_time_in"] = idx
                    out["image_index_to_time_out_" + fmt] = np.array([loader.image_index_to_time(int(i)) for i in idx])
                    ts = loader._image_cache["timestamp"]
                    times = np.concatenate([[0.0, ts[0], ts[0] + 1e-7, ts[2], ts[-1], ts[-1] + 1.0], rs.uniform(ts[0] - 0.004, ts[-1] + 0.004, 18)])
                    out.setdefault("time_to_image_index_in", times)
                    out["time_to_image_index_out_" + fmt] = np.array([int(loader.time_to_image_index(float(t)))
                                                                     for t in out["time_to_image_index_in"]])
                if fmt == "new":
                    continue
                calls.clear()
                got = [loader.load_image(i) for i in load_indices]
                if warp:
                    assert len(calls) == len(load_indices) and all(c[1] == (SENSOR[1], SENSOR[0]) for c in calls)
                    out["warp_dsize"] = np.array(calls[0][1])
                    out["warped_images"] = np.stack([g[0] for g in got])
                    assert out["warped_images"].shape[1:] == SENSOR
                else:
                    assert not calls
                    out["raw_images"] = np.stack([g[0] for g in got])
                    out["load_timestamps"] = np.array([g[1] for g in got])
                    out["load_indices"] = np.array(load_indices)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    assert np.array_equal(out["timestamps_old"], out["timestamps_new"]) and np.array_equal(out["raw_images"], frames[load_indices])
    path = os.path.join(HERE, "golden_frame_warp.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes): {sorted(out)}")


if __name__ == "__main__":
    warnings.filterwarnings("ignore")
    main()
