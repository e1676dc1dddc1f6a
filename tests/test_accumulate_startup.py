"""The accumulate pass's start-up after the split of the tile range (csrc/iwe_tile_core.h: tile_head / tile_bounds / tile_coords)
and the write-through IWE stores of the combine pass, at the smallest shapes where either can go wrong: tile grids whose width is
not a power of two, one tile, empty tiles, padded last groups, a partial last chunk, every way of cutting tiles into work items,
every built (tile, halo) pair, and the loops that read ``beg`` / ``end`` early (weights, (x, y, dt) format) or late (the checksum
that sends a slice to the f64 redo).

Images and variances are compared with the CPU oracle at the tolerance tests/test_gpu_parity.py uses for the slab path (rel-L2 of
the image < 1e-5, variance within 1e-5 relative: the fp32 slab sums against the fp64 reference); paths that share code are
compared bit for bit."""
import functools

import numpy as np
import pytest
import torch

from oracle import ebos_oracle as O

pytestmark = pytest.mark.gpu

SLAB_REL = 1e-5   # tests/test_gpu_parity.py: rel(iwe, ref) < 1e-5 on the slab path, variances to 1e-5 * |v|
FLOW_MAX = 5.0    # |dt| <= 1 (normalised time): every displacement stays inside the smallest built halo (8): nothing spills,
                  # so that every image is a sum of integers and bit-reproducible

# (image, tile, halo): 2 x 3 tiles (tiles_x not a power of two), 3 x 5, one tile
GEOMETRIES = [((90, 240), (45, 80), 32), ((135, 400), (45, 80), 32), ((32, 32), (32, 32), 8)]


@pytest.fixture(scope="module")
def ebos():
    import event_based_bos_amd as pkg

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg.load_library()
    return pkg


def G(a, dtype=None):
    t = torch.from_numpy(np.array(a)).to(torch.device("cuda:0"))  # (a copy: the shared inputs are read-only)
    return t if dtype is None else t.to(dtype)


def _tile_of(ev, size, tile):
    tiles_x = -(-size[1] // tile[1])
    return (ev[:, 0].astype(int) // tile[0]) * tiles_x + ev[:, 1].astype(int) // tile[1]


@functools.lru_cache(maxsize=None)
def _events(size, tile, kind, seed=7):
    """'random': ~3000 events, tile 1 and the last tile empty (where the grid has more than one tile), no tile's count a multiple
    of four (every tile's last group is padded); 'one_tile': 255 events in tile 0 (a partial last chunk of 64 groups);
    'blob': 20 000 events in a Gaussian blob at the image's centre (a plan whose heavy tiles are cut into parts)."""
    h, w = size
    rs = np.random.RandomState(seed)
    n_tiles = -(-h // tile[0]) * -(-w // tile[1])
    if kind == "blob":
        n = 20_000
        r = np.clip(np.rint(rs.normal(h / 2, 9.0, n)), 0, h - 1)
        c = np.clip(np.rint(rs.normal(w / 2, 9.0, n)), 0, w - 1)
        ev = np.stack([r, c, np.sort(rs.uniform(0, 0.5, n)), rs.randint(0, 2, n)], 1).astype(np.float64)
    elif kind == "one_tile":
        ev = O.synth_events(255, min(h, tile[0]), min(w, tile[1]), seed=seed)
    else:
        ev = O.synth_events(3000, h, w, seed=seed)
        t = _tile_of(ev, size, tile)
        if n_tiles > 1:
            ev = ev[(t != 1) & (t != n_tiles - 1)]
        t = _tile_of(ev, size, tile)
        drop = [int(np.flatnonzero(t == k)[0]) for k in range(n_tiles) if (t == k).sum() and (t == k).sum() % 4 == 0]
        ev = np.delete(ev, drop, axis=0)
        counts = np.bincount(_tile_of(ev, size, tile), minlength=n_tiles)
        assert np.all(counts[counts > 0] % 4 != 0)
        assert n_tiles == 1 or (counts == 0).sum() == 2
    ev.setflags(write=False)
    return ev


@functools.lru_cache(maxsize=None)
def _flow(size, seed=1):
    fl = O.synth_dense_flow(size[0], size[1], seed=seed, max_val=FLOW_MAX)
    fl.setflags(write=False)
    return fl


@functools.lru_cache(maxsize=None)
def _oracle(size, tile, kind, flow_seed=1):
    """(image, variance) of the CPU oracle: computed once per case, shared, never written to"""
    ev, fl = _events(size, tile, kind), _flow(size, flow_seed)
    iwe = O.iwe_dense(torch.from_numpy(ev.copy()), torch.from_numpy(fl.copy()), size)
    img = iwe.numpy()
    img.setflags(write=False)
    return img, abs(float(O.image_variance(iwe)))


def _slab(ebos, plan, flow, halo, splits, ws=None, weight=None, xy=False):
    """one call of the single-window entry (ebos_iwe_dense_slab_f32) -> (image, variance [1], workspace)"""
    from event_based_bos_amd import _hip

    lib = _hip.require_gpu()
    h, w = plan.image_size
    th, tw = plan.tile
    nws = int(lib.ebos_iwe_slab_workspace_bytes(h, w, th, tw, halo, splits, 0, 0))
    dev = flow.device
    if ws is None:
        ws = torch.zeros(nws, dtype=torch.uint8, device=dev)
    iwe = torch.empty((h, w), dtype=torch.float32, device=dev)
    out = torch.empty(1, dtype=torch.float32, device=dev)
    P = lambda t: None if t is None else t.data_ptr()
    cp = (None, None, None) if xy else plan._compact_ptrs()
    assert xy or cp[0] is not None
    _hip.check(lib.ebos_iwe_dense_slab_f32(P(plan.x), P(plan.y), P(plan.dt), P(weight), *cp, P(plan.key_offsets), plan.n, P(flow), h, w,
                                           th, tw, halo, splits, 0, 0, P(ws), nws, P(iwe), 1, 0, P(out), None, P(plan.part_table),
                                           _hip.stream_ptr()), "ebos_iwe_dense_slab")
    torch.cuda.synchronize()
    return iwe, out, ws


def _check(iwe, var, want_img, want_var, what):
    e_img = O.rel_l2(iwe.cpu().numpy(), want_img)
    e_var = abs(float(var) - want_var) / want_var
    print(f"{what}: image rel-L2 {e_img:.2e}  variance rel {e_var:.2e}")
    assert e_img < SLAB_REL and e_var < SLAB_REL, what


@pytest.mark.parametrize("kind", ["random", "one_tile"])
@pytest.mark.parametrize("size,tile,halo", GEOMETRIES)
def test_tile_grids_and_equal_splits_match_the_oracle(ebos, size, tile, halo, kind):
    """splits 1, 2, 3 on each grid: empty tiles, padded last groups, parts that get no group at all (255 events are 64 groups: the
    third part of three holds 20), against the oracle; the three images are sums of the same integers cut up differently."""
    ev = _events(size, tile, kind)
    plan = ebos.EventPlan.build(G(ev), size, "first", True, tile=tile, emit="compact")
    assert plan.compact and tuple(plan.tile) == tile
    flow = G(_flow(size), torch.float32)
    want_img, want_var = _oracle(size, tile, kind)
    for splits in (1, 2, 3):
        iwe, var, _ = _slab(ebos, plan, flow, halo, splits)
        _check(iwe, var, want_img, want_var, f"{size} {kind} splits {splits}")


@pytest.mark.parametrize("size,tile,halo", GEOMETRIES[:2])
def test_adaptive_work_items_match_the_oracle(ebos, size, tile, halo):
    """splits = 0 on a plan that ebos_plan_parts really splits: item_tile / item_part / part_off feed the head"""
    ev = _events(size, tile, "blob")
    plan = ebos.EventPlan.build(G(ev), size, "first", True, tile=tile, emit="compact")
    n_tiles = -(-size[0] // tile[0]) * -(-size[1] // tile[1])
    pt = plan.part_table.cpu().numpy()
    assert pt.shape[0] == 5 * n_tiles + 1
    parts = np.diff(pt[:n_tiles + 1])
    if parts.max() < 2:
        pytest.skip(f"ebos_plan_parts split no tile of this plan (parts per tile {parts.tolist()})")
    flow = G(_flow(size), torch.float32)
    want_img, want_var = _oracle(size, tile, "blob")
    iwe, var, _ = _slab(ebos, plan, flow, halo, 0)
    _check(iwe, var, want_img, want_var, f"{size} adaptive, parts per tile {parts.tolist()}")
    one, var1, _ = _slab(ebos, plan, flow, halo, 1)
    _check(one, var1, want_img, want_var, f"{size} blob, whole tiles")


def test_every_built_tile_and_halo(ebos):
    """each (tile, halo) pair the library was built with, on a grid of 2 x 2 tiles"""
    from event_based_bos_amd import _hip

    configs = _hip.slab_configs()
    assert configs
    for th, tw, halo in configs:
        size, tile = (2 * th, 2 * tw), (th, tw)
        plan = ebos.EventPlan.build(G(_events(size, tile, "random")), size, "first", True, tile=tile, emit="compact")
        want_img, want_var = _oracle(size, tile, "random")
        iwe, var, _ = _slab(ebos, plan, G(_flow(size), torch.float32), halo, 1)
        _check(iwe, var, want_img, want_var, f"tile {th} x {tw} halo {halo}")


@pytest.mark.parametrize("size,tile,halo", GEOMETRIES)
def test_second_call_on_a_workspace_does_not_show_the_first(ebos, size, tile, halo):
    """Two consecutive calls on ONE workspace with different flows: the second image equals, bit for bit, the one computed on a
    workspace of its own (slabs and -- since the combine pass stores the IWE write-through -- the image buffer's lines)."""
    plan = ebos.EventPlan.build(G(_events(size, tile, "random")), size, "first", True, tile=tile, emit="compact")
    fa, fb = G(_flow(size, 1), torch.float32), G(_flow(size, 2), torch.float32)
    want_a, var_a, _ = _slab(ebos, plan, fa, halo, 1)
    want_b, var_b, _ = _slab(ebos, plan, fb, halo, 1)
    assert not torch.equal(want_a, want_b)
    _, _, ws = _slab(ebos, plan, fa, halo, 1)
    for k in range(4):  # b, a, b, a on the workspace that held a
        fl, want, wvar = ((fb, want_b, var_b), (fa, want_a, var_a))[k % 2]
        got, var, _ = _slab(ebos, plan, fl, halo, 1, ws=ws)
        assert torch.equal(got, want) and torch.equal(var, wvar), k
    img_b, var_b2 = _oracle(size, tile, "random", 2)
    _check(want_b, var_b, img_b, var_b2, f"{size} second flow")


def test_per_event_weights_read_the_bounds_up_front(ebos):
    """weight != null: group_plan_index reads ``beg`` in the set-up and in the loop.  Against the oracle, and against its own
    second run bit for bit."""
    size, tile, halo = GEOMETRIES[0]
    ev = _events(size, tile, "random")
    plan = ebos.EventPlan.build(G(ev), size, "first", True, tile=tile)  # (the full build keeps the permutation)
    wgt = np.random.RandomState(3).uniform(0.5, 1.5, len(ev)).astype(np.float32)
    w_plan = ebos.event_plan._plan_weight(plan, G(wgt))
    flow = G(_flow(size), torch.float32)
    ref = O.iwe_dense(torch.from_numpy(ev.copy()), torch.from_numpy(_flow(size).copy()), size, weight=torch.from_numpy(wgt.astype(np.float64)))
    for splits in (1, 3):
        iwe, var, ws = _slab(ebos, plan, flow, halo, splits, weight=w_plan)
        _check(iwe, var, ref.numpy(), float(torch.var(ref)), f"weighted, splits {splits}")
        again, var2, _ = _slab(ebos, plan, flow, halo, splits, ws=ws, weight=w_plan)
        assert torch.equal(again, iwe) and torch.equal(var2, var), splits


def test_xy_dt_format(ebos):
    """cpix == null: the (x, y, dt) plan, whose groups are plan indices (the head reads key_offsets itself)"""
    size, tile, halo = GEOMETRIES[1]
    plan = ebos.EventPlan.build(G(_events(size, tile, "random")), size, "first", True, tile=tile)
    assert plan.x is not None
    want_img, want_var = _oracle(size, tile, "random")
    flow = G(_flow(size), torch.float32)
    for splits in (1, 2):
        iwe, var, _ = _slab(ebos, plan, flow, halo, splits, xy=True)
        _check(iwe, var, want_img, want_var, f"(x, y, dt) format, splits {splits}")


def test_nan_flow_takes_the_f64_redo(ebos):
    """One NaN flow value: the events of that pixel add nothing, the fixed-point checksum -- which reads ``beg`` / ``end`` behind
    the loop -- misses their units and the slice is redone in f64.  The image is the oracle's with those events masked out."""
    size, tile, halo = GEOMETRIES[0]
    ev = _events(size, tile, "random")
    r, c = int(ev[len(ev) // 2, 0]), int(ev[len(ev) // 2, 1])  # a pixel that holds an event
    fl = _flow(size).copy()
    fl[0, r, c] = np.nan
    keep = ~((ev[:, 0].astype(int) == r) & (ev[:, 1].astype(int) == c))
    assert 0 < (~keep).sum() < len(ev)
    ref = O.iwe_dense(torch.from_numpy(ev.copy()), torch.from_numpy(_flow(size).copy()), size, weight=torch.from_numpy(keep.astype(np.float64)))
    plan = ebos.EventPlan.build(G(ev), size, "first", True, tile=tile, emit="compact")
    for splits in (1, 2):
        iwe, var, _ = _slab(ebos, plan, G(fl, torch.float32), halo, splits)
        assert torch.isfinite(iwe).all()
        _check(iwe, var, ref.numpy(), float(torch.var(ref)), f"NaN flow at ({r}, {c}), splits {splits}")
