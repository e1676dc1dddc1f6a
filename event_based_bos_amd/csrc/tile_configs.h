// tile_configs.h -- the (tile_h, tile_w, halo) triples each tile-templated kernel family is built for, once per family, and what the
// C entry points derive from a list: the table ebos_*_config reports, the membership test, and the dispatcher that turns a run-time
// triple into template arguments.  Host code only; no kernels.
//
// To add or retire a triple, edit its line in the family's list below.  The slab family compiles one translation unit per triple:
// there, also add iwe_tiled_<TH>x<TW>x<HALO>.hip (one line: EBOS_DEFINE_SLAB_OPS) and its name in build.py's SOURCES.
// The order of a list is the order ebos_*_config reports, which the Python side sorts and filters: it is part of the behaviour.
//
// A triple that is not in its family's list:
//   refused, EBOS_ERR_UNSUPPORTED and "no kernel built for tile ... (see ebos_*_config)", before any launch:
//     ebos_iwe_dense_tiled_f32, ebos_iwe_voxel_tiled_f32, ebos_iwe_dense_multiref_tiled_f32 (and ebos_iwe_multiref_fits = 0), the
//     tangent entries of iwe_hvp.hip, every slab entry of iwe_tiled.hip and iwe_multiref_slab.hip (checked before the workspace
//     size); ebos_patch_fused_supported answers 0
//   runs on the general kernel instead, window by window: the two time-aware batch entries, ebos_iwe_voxel_tiled_batch_f32
//     (warp_voxel.hip) and multiref_tiled_batch (warp_voxel_multiref.hip)
// ebos_iwe_dense_tiled_f32 and ebos_iwe_voxel_tiled_f32 return EBOS_OK for n == 0 before they look at the triple; every other refusing
// entry checks the triple first.
#pragma once
#include "ebos_hip.h"

namespace ebos {

struct TileConfig {
  int th, tw, halo;
};

// a triple as a type: what a dispatcher hands its generic lambda, `[&](auto t) { return launch<t.th, t.tw, t.halo>(...); }`
template <int TH, int TW, int HL>
struct Tile {
  static constexpr int th = TH, tw = TW, halo = HL;
};

// LDS-atomic tiled family: iwe_fused.hip, warp_voxel.hip, warp_voxel_multiref.hip, iwe_multiref.hip, iwe_hvp.hip (ebos_tiled_config)
#define EBOS_TILED_CONFIGS(X) \
  X(64, 64, 32) X(32, 64, 32) X(32, 32, 32) X(64, 64, 16) X(32, 32, 16) X(32, 32, 8) X(64, 64, 64) X(32, 64, 48) X(16, 64, 32)

// slab family: iwe_tiled.hip and its per-triple units (ebos_slab_config)
// f64 tile + halo must fit 160 KiB (forward); backward needs 16 TH TW + 4 LH LW bytes
// {45, 80, 32} cuts 720 x 1280 into exactly 16 x 16 = 256 tiles: one workgroup per CU of an MI355X
// smaller halos for windows whose displacements are small (BOS flows are typically a few pixels): slabs, LDS clear / decode and
// the backward kernel's upstream tile all shrink with (TH + 2 halo)(TW + 2 halo); taps beyond the halo stay correct (spill)
#define EBOS_SLAB_CONFIGS(X) \
  X(64, 64, 32) X(45, 80, 32) X(32, 64, 32) X(32, 32, 32) X(64, 64, 16) X(45, 80, 16) X(32, 32, 16) X(32, 32, 8)

// multi-reference slab family: iwe_multiref_slab.hip (ebos_slab_multiref_config)
#define EBOS_MULTIREF_SLAB_CONFIGS(X) X(32, 32, 8) X(32, 32, 32) X(64, 64, 16) X(64, 64, 32)

// per family: TABLE, the list as a constexpr array; DISPATCH(th, tw, halo, f) = f(Tile<..>{}) of the matching triple, else
// EBOS_ERR_UNSUPPORTED
#define EBOS_TILE_ENTRY(TH, TW, HL) {TH, TW, HL},
#define EBOS_TILE_TRY(TH, TW, HL) \
  if (th == TH && tw == TW && halo == HL) return f(Tile<TH, TW, HL>{});
#define EBOS_TILE_FAMILY(TABLE, DISPATCH, LIST)        \
  constexpr TileConfig TABLE[] = {LIST(EBOS_TILE_ENTRY)}; \
  template <class F>                                   \
  int DISPATCH(int th, int tw, int halo, F&& f) {      \
    LIST(EBOS_TILE_TRY)                                \
    return EBOS_ERR_UNSUPPORTED;                       \
  }
EBOS_TILE_FAMILY(kTiledConfigs, dispatch_tiled, EBOS_TILED_CONFIGS)
EBOS_TILE_FAMILY(kSlabConfigs, dispatch_slab, EBOS_SLAB_CONFIGS)
EBOS_TILE_FAMILY(kMultirefSlabConfigs, dispatch_multiref_slab, EBOS_MULTIREF_SLAB_CONFIGS)
#undef EBOS_TILE_FAMILY
#undef EBOS_TILE_TRY
#undef EBOS_TILE_ENTRY

template <int N>
bool config_ok(const TileConfig (&table)[N], int th, int tw, int halo) {
  for (const TileConfig& c : table)
    if (c.th == th && c.tw == tw && c.halo == halo) return true;
  return false;
}

// what an ebos_*_config entry does: up to `cap` triples into `out` (which may be NULL), the number of built triples back
template <int N>
int copy_configs(const TileConfig (&table)[N], int* out, int cap) {
  for (int i = 0; i < N && i < cap && out != nullptr; ++i) {
    out[3 * i] = table[i].th;
    out[3 * i + 1] = table[i].tw;
    out[3 * i + 2] = table[i].halo;
  }
  return N;
}

}  // namespace ebos
