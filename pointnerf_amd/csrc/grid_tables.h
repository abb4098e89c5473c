// Host state of the persistent voxel grid: the handle, its
// device buffers, and the one statement of how their bytes are laid out and
// reused.  Included by grid.hip (the build), query.hip (the reader) and api.hip
// (the handle's lifetime) only.
#pragma once
#include "pnr_common.h"

// A device allocation that only grows.
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  int ensure(size_t want) {
    if (p && bytes >= want) return PNR_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
    if (hipMalloc(&p, want ? want : 16) != hipSuccess) {
      ::pnr::set_error("hipMalloc of %zu bytes failed", want);
      return PNR_ENOMEM;
    }
    bytes = want;
    return PNR_OK;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  template <typename T>
  T* as() const { return static_cast<T*>(p); }
};

// Grid geometry as the build and query kernels read it from device memory
// (GB_GEOM): written by the host (pnr_grid_build) or derived from the points'
// bbox on the device (pnr_grid_build_dev, no host sync).
struct QGrid {
  float shift[3], vs[3];
  int dims[3];
  int P;
};

// The handle's device buffers.  pnr_handle::buf is indexed by this enum, and
// the build's ensure pass and release_all walk it whole: a buffer exists by
// being listed here.  (gvol, words, max_o, N: GridLayout.)
enum GridBuf {
  GB_COOR_2_OCC,   // int32 [gvol]   cell -> slot, -1 = empty
  GB_OCC_BITS,     // uint32 [words] dilated occupancy bitmap
  GB_CELL_START,   // int32 [gvol]   first sorted position of the cell's run (occupied cells only)
  GB_CELL_END,     // int32 [gvol]   one past the last sorted position of the run; then zy_bytes()
  GB_CELL_BYTES,   // uint8: four regions, GridLayout::{occ,held,coarse,wrank}_off
  GB_OCC_NUMPNTS,  // int32 [max_o]  points that fell in the voxel
  GB_OCC_PTS,      // float4 [max_o*P] {x, y, z, bitcast(point id)}
  GB_OCC_2_COOR,   // int32 [max_o*3]
  GB_SORT_K0,      // uint32/uint64 [N] cell keys (ping-pong of the LSD radix sort)
  GB_SORT_K1,
  GB_SORT_V0,      // int32 [N]      point ids riding with the keys; the free one then claimers()
  GB_SORT_V1,
  GB_SORT_HIST,    // int32 [256*tiles + 1] per-tile digit counts
  GB_SORT_OFFS,    // int32 [256*tiles + 1] their exclusive scan
  GB_PT_FLAG,      // int32 [N]      1: the point claims a (kept) voxel
  GB_PT_SLOT,      // int32 [N+1]    exclusive scan of pt_flag
  GB_COUNTERS,     // int32 [8]
  GB_SEL,          // voxel reservoir: SelState, then sel_hist()
  GB_SCAN_TMP,     // scratch of exclusive_scan
  // Query index (what k_knn reads; the slot tables above stay the reference's
  // view for export / parity): the voxels that hold points, ranked in x-major
  // cell order, so a sample's 3x3x3 neighbourhood is found from a bitmap that
  // stays in L2 and its records sit near each other in HBM.
  GB_Q_WORDS,      // uint2 [words]  {bits: cell holds >= 1 kept point, rank of the word's first cell}
  GB_Q_WCNT,       // int32 [words+1] popcount per word (scratch)
  GB_Q_RANK_SLOT,  // int32 [max_o]  run_starts(), then the slot of rank r (scratch)
  GB_Q_RANK_CNT,   // int32 [max_o]  min(P, points) of rank r (scratch)
  GB_Q_REC_OFF,    // int32 [max_o+1] first record of rank r (exclusive scan of q_rank_cnt)
  GB_Q_RECS,       // float4 [N]     {x, y, z, bitcast(id)} in rank order, per voxel ascending id
  GB_GEOM,         // QGrid of the built grid
  GB_BBOX,         // float [8]  point bbox of a device-geometry build (no other build allocates it)
  GB_BBOX_ACC,     // uint32 [8] k_bbox's order-key accumulators, kept reset by k_geom_acc (likewise)
  kGridBufs
};

constexpr int kSelStateWords = 2;   // sizeof(SelState) / 4 (grid.hip asserts it)

// Sizes and offsets of one build, computed once (GridLayout::make, grid.hip)
// from the allocation-bound dims, max_o, P and n.  Everything that allocates,
// clears, carves or bounds a table reads it here.
struct GridLayout {
  int64_t gvol = 0;    // dims[0]*dims[1]*dims[2] of the allocation bound
  int64_t words = 0;   // ceil(gvol / 32)
  int64_t cap_o = 0;   // max_o
  int64_t n = 0;
  bool wide = false;   // uint64 cell keys: the sentinel key gvol does not fit uint32
  size_t bytes[kGridBufs] = {};   // 0: this build does not use the buffer
  // GB_CELL_BYTES = [occupancy bytes | held bytes | coarse column map | word ranks]
  //   occupancy bytes  uint8 [32*words]  k_claim, dilated in place, packed into GB_OCC_BITS
  //   held bytes       uint8 [32*words]  k_claim: the cell keeps >= 1 point; packed into GB_Q_WORDS
  //   coarse map       uint32 [ceil(dz/8)][dx][ceil(dy/32)], 16-B padded: bit y = column (x, y)
  //                    holds a kept point in z-block bz; k_claim writes, k_knn reads
  //   word ranks       int32 [words+1] (+ 12 B pad): exclusive scan of GB_Q_WCNT
  size_t occ_off = 0, held_off = 0, coarse_off = 0, wrank_off = 0;
  size_t clear_bytes = 0;   // the first three regions, cleared by one memset before k_claim
  int64_t wrank_cap = 0;    // int32 entries of the word-rank region
  static GridLayout make(const int dims[3], int64_t max_o, int P, int64_t n, bool device_geometry);
};

// What the build leaves for the host behind stats_ev: one pinned block, written
// by block 0 of the build's last kernel.
struct GridHostBlock {
  int32_t cnt[8];   // GB_COUNTERS
  QGrid geo;        // GB_GEOM: the exact geometry
  float bbox[8];    // GB_BBOX (device-geometry builds)
};

// Persistent grid tables owned by a handle.
struct pnr_handle {
  int device = 0;
  DevBuf buf[kGridBufs];
  GridLayout lay;              // of the last build
  // what later calls need of the last build
  int bound_dims[3] = {};      // allocation bound of the tables: >= the exact dims (equal on a host-geometry build)
  int max_o = 0, P = 0;
  bool geom_on_device = false; // the exact geometry was derived on the device: only GB_GEOM / host->geo hold it
  bool bbox_acc_ready = false; // GB_BBOX_ACC holds its initial state (k_bbox_acc_init ran on this allocation)
  pnr_grid_stats stats{};
  bool built = false;          // false from a build's first allocation until its last launch succeeded
  // build results read back without blocking the build: pinned block + event,
  // waited on by pnr_grid_stats_get / pnr_grid_geometry / pnr_grid_bbox only
  GridHostBlock* host = nullptr;
  hipEvent_t stats_ev = nullptr;
  bool stats_pending = false;

  template <typename T>
  T* tab(int b) const { return buf[b].as<T>(); }   // b: a GridBuf
  uint8_t* cell_bytes(size_t off) const { return buf[GB_CELL_BYTES].as<uint8_t>() + off; }
  // Storage with a second use inside one build, each live only where stated:
  // GB_CELL_END after k_claim read the run ends: the zy-dilated bytes (k_dilate_zy -> k_dilate_x)
  uint8_t* zy_bytes() const { return buf[GB_CELL_END].as<uint8_t>(); }
  // GB_Q_RANK_SLOT from k_claim to k_reservoir: slot -> start of its run; k_rank_slots overwrites it
  int32_t* run_starts() const { return buf[GB_Q_RANK_SLOT].as<int32_t>(); }
  // the sort's value buffer that does not hold the result (cur: the one that does), free after
  // the last pass: the voxel reservoir's claimer list (k_sel_hist pass 0 -> k_sel_apply)
  int32_t* claimers(int cur) const { return buf[GB_SORT_V0 + (cur ^ 1)].as<int32_t>(); }
  // GB_SEL behind its SelState: kSelPasses x 256 bins, zeroed by k_cell_keys when n > max_o
  uint32_t* sel_hist() const { return buf[GB_SEL].as<uint32_t>() + kSelStateWords; }

  void release_all() {
    if (host) (void)hipHostFree(host);
    host = nullptr;
    if (stats_ev) (void)hipEventDestroy(stats_ev);
    stats_ev = nullptr;
    stats_pending = false;
    built = bbox_acc_ready = false;
    for (DevBuf& b : buf) b.release();
  }
};
