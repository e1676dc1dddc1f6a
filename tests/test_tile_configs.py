"""CPU checks of the built (tile_h, tile_w, halo) triples (csrc/tile_configs.h): the three ``ebos_*_config`` entries and their order, the
cached Python readers, the slab family's per-triple units in ``build.SOURCES``, ``ebos_patch_fused_supported`` on a recorded grid, and
the refusal of an unbuilt triple by an entry of every family (before any HIP call: usable without a GPU)."""
import ctypes
import re

import pytest

TILED = [(64, 64, 32), (32, 64, 32), (32, 32, 32), (64, 64, 16), (32, 32, 16), (32, 32, 8), (64, 64, 64), (32, 64, 48), (16, 64, 32)]
SLAB = [(64, 64, 32), (45, 80, 32), (32, 64, 32), (32, 32, 32), (64, 64, 16), (45, 80, 16), (32, 32, 16), (32, 32, 8)]
MULTIREF_SLAB = [(32, 32, 8), (32, 32, 32), (64, 64, 16), (64, 64, 32)]

# ebos_patch_fused_supported(th, tw, halo, slide_h, slide_w): one string per slide_h, one digit per slide_w, both over SLIDES.  Recorded
# from the library as it was before the triples moved into tile_configs.h.
SLIDES = (1, 4, 8, 16, 45, 80)
HALO_AUTO_32 = -16416  # EBOS_HALO_AUTO(32, 64): run-time windows of at most the built halo 32, |dt| <= 1
HALO_AUTO_24 = -16408  # ... of at most 24, which no triple is built with
FUSED_SUPPORTED = {
    (64, 64, 32): ("000000", "000000", "000000", "000000", "000000", "000000"),
    (45, 80, 32): ("000000", "001111", "001111", "001111", "001111", "001111"),
    (32, 64, 32): ("000000", "001111", "001111", "001111", "001111", "001111"),
    (32, 32, 32): ("000000", "011111", "011111", "011111", "011111", "011111"),
    (64, 64, 16): ("000000", "000000", "001111", "001111", "001111", "001111"),
    (45, 80, 16): ("000000", "001111", "001111", "001111", "001111", "001111"),
    (32, 32, 16): ("000000", "011111", "011111", "011111", "011111", "011111"),
    (32, 32, 8): ("000000", "011111", "011111", "011111", "011111", "011111"),
    (33, 32, 8): ("000000",) * 6,                                                          # not built
    (64, 64, HALO_AUTO_32): ("000000",) * 6,                                               # as (64, 64, 32)
    (45, 80, HALO_AUTO_32): ("000000", "001111", "001111", "001111", "001111", "001111"),  # as (45, 80, 32)
    (32, 32, HALO_AUTO_24): ("000000",) * 6,                                               # not built
}


@pytest.fixture(scope="module")
def lib():
    from event_based_bos_amd import _hip
    from event_based_bos_amd.build import build_library

    build_library(verbose=False)
    return _hip.load_library()


@pytest.mark.parametrize("entry, want", [("ebos_tiled_config", TILED), ("ebos_slab_config", SLAB), ("ebos_slab_multiref_config", MULTIREF_SLAB)])
def test_config_entries_report_the_lists_in_order(lib, entry, want):
    fn = getattr(lib, entry)
    n = len(want)
    assert fn(None, 0) == n and fn(None, n) == n                                           # out = NULL: the count
    flat = [v for t in want for v in t]
    buf = (ctypes.c_int * (3 * n + 3))(*([-7] * (3 * n + 3)))
    assert fn(buf, n) == n and list(buf) == flat + [-7] * 3
    buf = (ctypes.c_int * (3 * n + 3))(*([-7] * (3 * n + 3)))
    assert fn(buf, n + 1) == n and list(buf) == flat + [-7] * 3                            # a larger cap writes no more than there is
    for cap in (0, 1, n - 1):
        buf = (ctypes.c_int * (3 * n))(*([-7] * (3 * n)))
        assert fn(buf, cap) == n                                                           # still the full count
        assert list(buf) == flat[:3 * cap] + [-7] * (3 * (n - cap))                        # only `cap` triples written


def test_python_readers_are_stable_and_hand_out_fresh_lists(lib):
    from event_based_bos_amd import _hip

    for reader, want in ((_hip.tiled_configs, TILED), (_hip.slab_configs, SLAB), (_hip.slab_multiref_configs, MULTIREF_SLAB)):
        first = reader()
        assert first == want and type(first) is list and all(type(t) is tuple for t in first)
        assert reader() == first and reader() is not first
        first.append((1, 2, 3))
        first[0] = (0, 0, 0)
        assert reader() == want


def test_slab_units_in_the_build_list_are_the_slab_triples(lib):
    from event_based_bos_amd import _hip, build

    units = [re.fullmatch(r"iwe_tiled_(\d+)x(\d+)x(\d+)\.hip", s) for s in build.SOURCES]
    units = [tuple(int(v) for v in m.groups()) for m in units if m]
    assert len(units) == len(set(units)) and set(units) == set(_hip.slab_configs())


def test_patch_fused_supported_is_what_it_was(lib):
    assert lib.ebos_halo_auto(32, 1.0) == HALO_AUTO_32 and lib.ebos_halo_auto(24, 1.0) == HALO_AUTO_24
    assert {t for t in FUSED_SUPPORTED if t[2] >= 0 and t != (33, 32, 8)} == set(SLAB)
    for (th, tw, hl), rows in FUSED_SUPPORTED.items():
        got = tuple("".join(str(lib.ebos_patch_fused_supported(th, tw, hl, sh, sw)) for sw in SLIDES) for sh in SLIDES)
        assert got == rows, (th, tw, hl)
    for sh, sw in ((0, 8), (8, 0), (0, 0), (-1, 8)):
        assert lib.ebos_patch_fused_supported(32, 32, 8, sh, sw) == 0


def _refusal(lib, rc, text):
    assert rc == -3 and lib.ebos_last_error().decode() == text                            # -3 = EBOS_ERR_UNSUPPORTED


def test_tiled_family_refuses_an_unbuilt_triple(lib):
    p = 0x1000
    dense = lambda n, th: lib.ebos_iwe_dense_tiled_f32(p, p, p, None, p, n, p, 37, 70, th, 32, 8, 1, 0, 0, p, None)  # noqa: E731
    _refusal(lib, dense(10, 33), "ebos_iwe_dense_tiled: no kernel built for tile 33x32 halo 8 (see ebos_tiled_config)")
    assert dense(0, 33) == 0                                                               # n == 0 returns before the triple is looked at
    voxel = lambda n, th: lib.ebos_iwe_voxel_tiled_f32(p, p, p, None, p, p, n, p, 5, 37, 70, th, 32, 8, 1, 0, 0, p, None)  # noqa: E731
    _refusal(lib, voxel(10, 33), "ebos_iwe_voxel_tiled: no kernel built for tile 33x32 halo 8 (see ebos_tiled_config)")
    assert voxel(0, 33) == 0
    shifts = (ctypes.c_float * 1)(0.25)
    multi = lambda n: lib.ebos_iwe_dense_multiref_tiled_f32(p, p, p, p, n, p, 37, 70, 33, 32, 8, 1, 0, 0, shifts, 1, p, None)  # noqa: E731
    text = ("ebos_iwe_dense_multiref_tiled: 1 windows of tile 33x32 halo 8 do not fit the LDS, or no kernel is built for it "
            "(see ebos_iwe_multiref_fits, ebos_tiled_config)")
    _refusal(lib, multi(10), text)
    _refusal(lib, multi(0), text)                                                          # here the triple comes before n == 0
    assert lib.ebos_iwe_multiref_fits(33, 32, 8, 1) == 0 and lib.ebos_iwe_multiref_fits(45, 80, 32, 1) == 0   # a slab triple is no tiled one
    tangent = lambda n, iwe: lib.ebos_iwe_dense_tangent_tiled_f32(p, p, p, p, n, p, p, 37, 70, 33, 32, 8, 1, 0, 0, iwe, p, None)  # noqa: E731
    _refusal(lib, tangent(10, None), "ebos_iwe_dense_tangent_tiled: 1 window(s) of tile 33x32 halo 8 do not fit the LDS, or no kernel is built "
                                     "for it (see ebos_iwe_multiref_fits, ebos_tiled_config)")
    _refusal(lib, tangent(0, p), "ebos_iwe_dense_tangent_tiled: 2 window(s) of tile 33x32 halo 8 do not fit the LDS, or no kernel is built "
                                 "for it (see ebos_iwe_multiref_fits, ebos_tiled_config)")
    _refusal(lib, lib.ebos_iwe_dense_tangent_slab_f32(p, p, p, p, 10, p, p, 37, 70, 33, 32, 8, 0, 0, p, 1 << 30, None, p, None),
             "ebos_iwe_dense_tangent_slab: 1 window(s) of tile 33x32 halo 8 do not fit the LDS, or no kernel is built for it "
             "(see ebos_iwe_multiref_fits, ebos_tiled_config)")


def test_slab_family_refuses_an_unbuilt_triple_before_the_workspace_size(lib):
    p = 0x1000

    def fwd(th, tw, hl, ws_bytes):
        return lib.ebos_iwe_dense_slab_f32(p, p, p, None, None, None, None, p, 10, p, 37, 70, th, tw, hl, 1, 0, 0, p, ws_bytes, p, 0, 0, None,
                                           None, None, None)

    _refusal(lib, fwd(33, 32, 8, 0), "ebos_iwe_dense_slab: no kernel built for tile 33x32 halo 8 (see ebos_slab_config)")
    _refusal(lib, fwd(16, 64, 32, 0), "ebos_iwe_dense_slab: no kernel built for tile 16x64 halo 32 (see ebos_slab_config)")   # a tiled triple
    _refusal(lib, fwd(32, 32, HALO_AUTO_24, 0), "ebos_iwe_dense_slab: no kernel built for tile 32x32 halo 24 (see ebos_slab_config)")
    assert fwd(32, 32, 8, 0) == -4 and b"workspace too small" in lib.ebos_last_error()     # built: the next check (-4 = EBOS_ERR_SCRATCH)
    rc = lib.ebos_iwe_dense_tiled_bwd_f32(p, p, p, None, None, None, None, p, 10, p, 37, 70, 33, 32, 8, 0, 0, p, None, 0, p, None, None, None,
                                          None, None, 0, None, None)
    _refusal(lib, rc, "ebos_iwe_dense_tiled_bwd: no kernel built for tile 33x32 halo 8 (see ebos_slab_config)")


def test_multiref_slab_family_refuses_a_slab_triple_it_is_not_built_for(lib):
    p = 0x1000
    shifts = (ctypes.c_float * 2)(0.0, -1.0)
    for th, tw, hl in ((45, 80, 32), (45, 80, 16), (33, 32, 8)):
        rc = lib.ebos_iwe_dense_slab_multiref_f32(p, p, p, p, 10, p, 37, 70, th, tw, hl, 1, 0, 0, shifts, 2, p, 0, p, 0, 0, None, None, None)
        _refusal(lib, rc, f"ebos_iwe_dense_slab_multiref: no kernel built for tile {th}x{tw} halo {hl} (see ebos_slab_multiref_config)")
        rc = lib.ebos_iwe_dense_tiled_multiref_bwd_f32(p, p, p, p, 10, p, 37, 70, th, tw, hl, 0, 0, shifts, 2, p, None, 0, None, None, None, None,
                                                       p, None)
        _refusal(lib, rc, f"ebos_iwe_dense_tiled_multiref_bwd: no kernel built for tile {th}x{tw} halo {hl} (see ebos_slab_multiref_config)")
        assert lib.ebos_iwe_slab_multiref_workspace_bytes(2, 37, 70, th, tw, hl, 1, 0, 0) == 0
