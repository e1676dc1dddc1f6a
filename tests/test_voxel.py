"""CPU checks of the event voxel port (event_based_bos_amd/event_voxel.py, csrc/event_voxel.hip): no kernel runs here.

* tests/_voxel_ref.py -- the numpy restatement the GPU tests compare the kernels with -- reproduces tests/golden/golden_voxel.npz,
  the arrays the REFERENCE's ``create_event_voxel`` and ``generate_discretized_event_volume`` gave, exactly: both add a voxel's
  votes sequentially in one order.  The one exception is the normalised grid: its mean and std are sums over ~800 voxels that
  torch and numpy add in different orders, so that case is held to the project's float64 image bar (rel-L2 <= 1e-12) on an
  equal non-zero mask, and its un-normalised grid exactly.
* ``utils`` and the package root export both reference names with the reference's parameters (tests/golden/voxel_signatures.json).
* Argument errors are raised before any GPU work, and the header and the ctypes table agree on the new entries.
"""
import inspect
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import _voxel_ref as R  # noqa: E402

G = np.load(os.path.join(HERE, "golden", "golden_voxel.npz"))
SIG = json.load(open(os.path.join(HERE, "golden", "voxel_signatures.json")))
SHAPE = tuple(int(v) for v in G["shape"])
VOL = tuple(int(v) for v in G["vol_size"])
ENTRIES = ("ebos_event_voxel_f64", "ebos_event_voxel_normalize_scratch_bytes", "ebos_event_voxel_normalize_f64",
           "ebos_event_volume_f64", "ebos_event_volume_f32", "ebos_event_voxel_raw_batch")


def case(c):
    return tuple(G[f"{c}_{k}"] for k in ("x", "y", "pol", "t"))


@pytest.mark.parametrize("c", ["int", "frac", "pos"])
def test_restatement_reproduces_the_reference_grid(c):
    grid, k, sabs = R.create_event_voxel(*case(c), SHAPE)
    want = G[f"{c}_grid"]
    assert grid.shape == want.shape == SHAPE and grid.dtype == np.float64
    assert np.array_equal(grid, want), int((grid != want).sum())
    assert (grid[k == 0] == 0).all() and (np.abs(grid) <= sabs).all()
    assert np.all(np.diff(G[f"{c}_t"]) > 0)
    if c == "frac":   # the coordinates the trilinear masks are there for
        x, y = G["frac_x"], G["frac_y"]
        assert ((x > -1) & (x < 0)).any() and ((y > -1) & (y < 0)).any() and (x > SHAPE[2] - 1).any() and (y > SHAPE[1] - 1).any()
    if c == "int":
        assert np.array_equal(G["int_x"], np.trunc(G["int_x"])) and set(G["int_pol"]) == {-1.0, 1.0}


def test_restatement_reproduces_the_reference_normalisation():
    got, want = R.normalize_voxel(G["pos_grid"]), G["pos_grid_normalized"]
    assert set(G["pos_pol"]) == {1.0}
    assert np.array_equal(got != 0, want != 0) and np.array_equal(want != 0, G["pos_grid"] != 0)
    err = np.linalg.norm(got - want) / np.linalg.norm(want)
    print(f"normalised grid: rel-L2 {err:.3e} to the reference's")
    assert err <= 1e-12
    nz = want[want != 0]
    assert abs(nz.mean()) < 1e-12 and abs(nz.std(ddof=1) - 1.0) < 1e-12
    # a grid without a non-zero voxel stays as it is; a single voxel (std is NaN) and equal voxels (std 0) are centred only
    assert np.array_equal(R.normalize_voxel(np.zeros((2, 3, 4))), np.zeros((2, 3, 4)))
    one = np.zeros((2, 3, 4))
    one[1, 2, 3] = 5.0
    assert np.array_equal(R.normalize_voxel(one), np.zeros((2, 3, 4)))
    two = np.zeros((2, 3, 4))
    two[0, 0, 0] = two[1, 1, 1] = 2.5
    assert np.array_equal(R.normalize_voxel(two), np.zeros((2, 3, 4)))


@pytest.mark.parametrize("c,dtype", [("vol", np.float64), ("vol32", np.float32)])
def test_restatement_reproduces_the_reference_volume(c, dtype):
    ev = G[f"{c}_events"]
    vol, k, sabs = R.generate_discretized_event_volume(ev, VOL)
    want = G[f"{c}_volume"]
    assert ev.dtype == dtype and vol.dtype == want.dtype == dtype and vol.shape == VOL
    assert np.array_equal(vol, want), int((vol != want).sum())
    assert (ev[:, 3] < 0).any() and (ev[:, 3] > 0).any()
    nb = VOL[0] // 2
    assert vol[:nb].sum() > 0 and vol[nb:].sum() > 0 and (vol[k == 0] == 0).all()


def params_of(fn):
    return [[p.name, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
            for p in inspect.signature(fn).parameters.values()]


def test_utils_and_the_package_export_the_reference_names():
    import event_based_bos_amd as ebos
    from event_based_bos_amd import event_voxel

    assert sorted(SIG) == ["create_event_voxel", "generate_discretized_event_volume"]
    for name, rec in SIG.items():
        for where in (ebos.utils, ebos, event_voxel):
            assert params_of(getattr(where, name)) == rec["params"], (where.__name__, name)
        assert getattr(ebos.utils, name) is getattr(event_voxel, name)
    assert [p[0] for p in params_of(ebos.event_voxel_batch)][:7] == ["columns", "ranges", "n_bins", "image_shape", "roi", "signed",
                                                                      "normalize"]
    assert [p[0] for p in params_of(ebos.RawEventStore.voxels)][:3] == ["self", "ranges", "n_bins"]
    assert "ValueError" in event_voxel.create_event_voxel.__doc__ and "ValueError" in event_voxel.generate_discretized_event_volume.__doc__


def test_single_call_argument_errors_come_before_any_gpu_work(monkeypatch):
    from event_based_bos_amd import _hip, event_voxel as V

    def no_gpu():
        raise AssertionError("the GPU was asked for before the arguments were checked")

    monkeypatch.setattr(_hip, "require_gpu", no_gpu)
    a = np.zeros(5)
    with pytest.raises(ValueError, match="one shape"):
        V.create_event_voxel(a, a, a, np.zeros(4), (5, 12, 16))
    with pytest.raises(ValueError, match="1-D"):
        V.create_event_voxel(*(np.zeros((5, 1)),) * 4, (5, 12, 16))
    with pytest.raises(ValueError, match="1-D"):
        V.create_event_voxel(*(torch.zeros(()),) * 4, (5, 12, 16))
    for shape in ((0, 12, 16), (5, 12), (5, 0, 16), (5.5, 12, 16), 5):
        with pytest.raises(ValueError, match="voxel_shape"):
            V.create_event_voxel(a, a, a, a, shape)
    with pytest.raises(ValueError, match="no events"):
        V.create_event_voxel(*(np.zeros(0),) * 4, (5, 12, 16))
    with pytest.raises(ValueError, match=r"\[n, 4\]"):
        V.generate_discretized_event_volume(np.zeros((5, 3)), (6, 12, 16))
    with pytest.raises(ValueError, match=r"\[n, 4\]"):
        V.generate_discretized_event_volume(np.zeros(4), (6, 12, 16))
    for size in ((1, 12, 16), (6, 12), (6, 0, 16)):
        with pytest.raises(ValueError, match="vol_size"):
            V.generate_discretized_event_volume(np.zeros((5, 4)), size)
    with pytest.raises(ValueError, match="no events"):
        V.generate_discretized_event_volume(np.zeros((0, 4)), (6, 12, 16))


def test_batch_argument_errors_come_before_any_gpu_work(monkeypatch):
    from event_based_bos_amd import _hip, event_voxel as V

    def no_gpu():
        raise AssertionError("the GPU was asked for before the arguments were checked")

    monkeypatch.setattr(_hip, "require_gpu", no_gpu)
    n = 10
    cols = (torch.zeros(n, dtype=torch.int16), torch.zeros(n, dtype=torch.int16), torch.arange(n, dtype=torch.int32),
            torch.zeros(n, dtype=torch.uint8))
    ok = dict(ranges=[(0, 10)], n_bins=5, image_shape=(12, 16))

    def call(columns=cols, **kw):
        return V.event_voxel_batch(columns, **{**ok, **kw})

    with pytest.raises(ValueError, match="int16"):
        call((cols[0].float(),) + cols[1:])
    with pytest.raises(ValueError, match="ticks"):
        call(cols[:2] + (cols[2].double(),) + cols[3:])
    with pytest.raises(ValueError, match="uint8 or bool"):
        call(cols[:3] + (cols[3].float(),))
    with pytest.raises(ValueError, match="equal length"):
        call(cols[:3] + (cols[3][:4],))
    with pytest.raises(ValueError, match="equal length"):
        call(tuple(c.reshape(2, 5) for c in cols))
    for bins in (0, -1, 2.5):
        with pytest.raises(ValueError, match="n_bins"):
            call(n_bins=bins)
    for ranges in ([], [(0, 11)], [(-1, 4)], [(11, 11)], [(0, 4, 5)], [3]):
        with pytest.raises(ValueError, match="range"):
            call(ranges=ranges)
    with pytest.raises(ValueError, match="image_shape"):
        call(image_shape=(12, 0))
    for roi in ((2, 2, 0, 16), (0, 13, 0, 16), (0, 12, -1, 16), (4, 2, 0, 16), (0, 12, 0), (0.5, 12, 0, 16),
                {"xmin": 0, "xmax": 12, "ymin": 3, "ymax": 17}):
        with pytest.raises(ValueError, match="roi"):
            call(roi=roi)
    with pytest.raises(ValueError, match="ticks_per_second"):
        call(ticks_per_second=0.0)
    with pytest.raises(ValueError, match="on the GPU"):       # everything else is in order: the CPU columns are what is left to refuse
        call(ranges=[(4, 2), (0, 0), (0, 10)], roi={"xmin": 0, "xmax": 12, "ymin": 3, "ymax": 16})
    store_cols = {"x": np.zeros(n, np.int16), "y": np.zeros(n, np.int16), "t": np.arange(n, dtype=np.int32), "p": np.zeros(n, bool)}
    from event_based_bos_amd import RawEventStore

    with pytest.raises(IndexError):
        RawEventStore(store_cols).voxels([(0, 11)], 5, (12, 16))
    with pytest.raises(ValueError, match="no window"):
        RawEventStore(store_cols).voxels([], 5, (12, 16))


def test_header_and_ctypes_entries_agree():
    from event_based_bos_amd import _hip, build

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ebos_hip.h")).read(), flags=re.S)
    for name in ENTRIES:
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert m, f"{name} is not declared in ebos_hip.h"
        assert name in _hip.SIGNATURES, f"{name} is not in the ctypes table"
        assert m.group(1).count(",") + 1 == len(_hip.SIGNATURES[name][1]), name
    for macro, value in (("EBOS_EVENT_VOLUME_OUT_OF_BOUNDS", _hip.EVENT_VOLUME_OUT_OF_BOUNDS),
                         ("EBOS_EVENT_VOLUME_DEGENERATE_SPAN", _hip.EVENT_VOLUME_DEGENERATE_SPAN)):
        assert re.search(r"#define\s+" + macro + r"\s+" + str(value) + r"\b", text), macro
    assert _hip.ABI_VERSION == 2                                   # entries were only added
    assert "event_voxel.hip" in build.SOURCES and "-ffp-contract=off" in build.PER_FILE_FLAGS["event_voxel.hip"]


def test_library_exports_the_entries_and_checks_arguments_on_the_host():
    from event_based_bos_amd import _hip
    from event_based_bos_amd.build import build_library

    build_library(verbose=False)
    lib = _hip.load_library()
    for name in ENTRIES:
        assert hasattr(lib, name), name
    assert lib.ebos_event_voxel_normalize_scratch_bytes(1) == 256 * 24 and lib.ebos_event_voxel_normalize_scratch_bytes(3) == 3 * 256 * 24
    assert lib.ebos_event_voxel_normalize_scratch_bytes(0) == 0
    # argument validation happens before any HIP call: usable without a GPU
    assert lib.ebos_event_voxel_f64(None, None, None, None, 5, 5, 12, 16, None, None, None) == -1
    assert b"NULL buffer" in lib.ebos_last_error()
    assert lib.ebos_event_volume_f32(None, 5, 6, 12, 16, None, None, None) == -1
    assert lib.ebos_event_voxel_normalize_f64(0, 10, None, None, 0, None) == -1
    assert lib.ebos_event_voxel_raw_batch(None, None, None, 0, None, 0, 1e6, None, 0, 0, 5, 12, 16, 0, 0, 0, 0, 0, 1, None, None, None,
                                          None) == -1
    assert b"windows" in lib.ebos_last_error()
