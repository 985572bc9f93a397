/* csrc/mfma_front.h -- what the four matrix-core channelizers of stage 1 share whatever their staging and number format (channelizer_dft.hip,
 * channelizer_dft_wide.hip: int8, which get it through dft_common.h; channelizer_f32.hip, channelizer_f32_wide.hip: float32): which work item a workgroup takes and
 * where on the chip, its range of 16-hop tiles and its share of them, the float pair's exchange of partial sums, and on the host the opt-in to more than 64 KiB of
 * dynamic LDS.  The int8 pair's TileAcc and piece sum are in dft_common.h.
 *
 * The device helpers are __forceinline__ and take the FIELDS they need BY VALUE, never the kernel-argument struct by reference: a helper that is handed the struct
 * compiles to different instruction counts than the text it replaces, one that is handed values only reorders (profiles/front_refactor.md).
 *
 * NOT here, though the four files hold it four times: the lane's ring view and the ring-store epilogue.  Written as by-value helpers (ring_lane(), store_tile<INT8>())
 * and tried on every one of the four files, each of the two moves vector-register counts or instruction counts in every file -- store_tile(): VGPRs +-2 in 28 of 74
 * dft, 28 of 68 dft_wide and 18 of 32 f32 kernels, one s_add_i32 and one v_add_u32 more in all 6 f32_wide kernels -- so by the rule that no kernel's registers or
 * counts move for the sake of sharing, the copies stay; the same file has the figures, and those of the float B load and MFMA loop. */
#ifndef AIRBAND_CSRC_MFMA_FRONT_H
#define AIRBAND_CSRC_MFMA_FRONT_H

#include <hip/hip_runtime.h>
#include <atomic>
#include <cstddef>
#include <stdint.h>

#include "common.h"

namespace airband {

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int TILE_HOPS = 16;

/* ---- work items ---- */

/* A work item = (dongle, group of 8 channels): dongles with more than 8 channels appear once per group, side by side, so the groups of a dongle stream the same
 * bytes at the same time through the same L2.  Workgroup b takes item b % n_items of tile-range split b / n_items (split >= the launch's splits: nothing to do).
 * XCD-aware placement: workgroup b runs on XCD b % 8 (observed dispatch order; speed only).  16 consecutive dongles write neighbouring slots of the same 128-byte
 * lines, so they are given to the SAME XCD and meet in one L2: inside every group of 128 items, workgroup i*8 + x takes item x*16 + i. */
struct WorkItem {
    int item, split;
};
__device__ __forceinline__ WorkItem work_item(int wg, int n_items) { /* wg: blockIdx.x */
    const int i_lin = wg % n_items;
    const int g128 = i_lin & ~127, in128 = i_lin & 127;
    WorkItem w;
    w.item = ((n_items - g128) >= 128) ? g128 + (in128 & 7) * 16 + (in128 >> 3) : i_lin;
    w.split = wg / n_items;
    return w;
}

/* MFMA tiles are aligned to the 16-row tiles of the output rings: tile t covers hops [16 t - shift, 16 t - shift + 16) and lands at physical 16-row tile
 * (ptile0 + t) mod ring_tiles16; hops < 0 (first tile) and >= n_hops (last tile) are computed on whatever bytes are there and never stored */
struct TileRange {
    int shift, ring_tiles, ring_tiles16, ptile0, tiles_total;
};
__device__ __forceinline__ TileRange tile_range(int row0, int first_row, int ring_rows, int n_hops) {
    TileRange g;
    g.shift = (row0 + first_row) & 15;
    g.ring_tiles = ring_rows / AB_TILE_ROWS;
    g.ring_tiles16 = ring_rows / TILE_HOPS; /* the ring length is a whole number of 16-hop MFMA tiles */
    g.ptile0 = (row0 + first_row) >> 4;
    g.tiles_total = (g.shift + n_hops + TILE_HOPS - 1) / TILE_HOPS;
    return g;
}
/* split `split` of `splits` equal shares of [0, total) -- tiles, or channelizer_dft.hip's staging steps; begin >= end: an empty share */
struct Share {
    int begin, end;
};
__device__ __forceinline__ Share split_share(int total, int splits, int split) {
    const int per_split = (total + splits - 1) / splits;
    Share r;
    r.begin = split * per_split;
    r.end = min(total, r.begin + per_split);
    return r;
}

/* ---- the float pair's exchange ---- */
/* ---- the float pair's contraction and exchange ---- */
/* One workgroup of NW waves per work item; wave `piece` owns an NW-th of the contraction index and one wave, `fin` (which one rotates with the workgroup), adds the
 * partial sums up and writes the rings. */
/* The other waves' partial sums reach the finishing wave through LDS, exch = [tile parity][NW - 1][64]: two areas alternate, so that a wave a tile ahead never
 * overwrites what the finishing wave still adds up.  put: every other wave, in front of the tile's barrier; sum: the finishing wave, behind it. */
template <int NW>
__device__ __forceinline__ float4* f32_exchange_put(float4* exch, int t, int piece, int fin, int lane, const v4f& acc) {
    float4* ex = exch + (t & 1) * (NW - 1) * 64;
    if (piece != fin) ex[((piece - fin - 1) & (NW - 1)) * 64 + lane] = make_float4(acc[0], acc[1], acc[2], acc[3]);
    return ex;
}
template <int NW>
__device__ __forceinline__ void f32_exchange_sum(const float4* ex, int lane, float* val) {
#pragma unroll
    for (int q = 0; q < NW - 1; q++) {
        const float4 o = ex[q * 64 + lane];
        val[0] += o.x; val[1] += o.y; val[2] += o.z; val[3] += o.w;
    }
}

/* ---- host: more than the default 64 KiB of dynamic LDS ---- */

/* A CU's whole LDS, 163 840 bytes.  dft_wide_map.h's WIDE_LDS_MAX and f32_wide_map.h's F32W_LDS_MAX, the ceilings the wide kernels' plans are cut to, are this
 * same number (their kernels' files assert it), so every variant asks for it. */
constexpr int CU_LDS_BYTES = 160 * 1024;
constexpr int BIG_LDS_DEVICES = 64;

/* Call in front of a launch of kernel `fn` with `lds` bytes of dynamic LDS: more than the default 64 KiB needs an opt-in.  done_for_device: BIG_LDS_DEVICES
 * zero-initialised flags of that kernel variant -- the attribute belongs to the function as loaded on the current device, and a process may drive several GPUs, so
 * once per variant AND device.  It asks for the CU's whole LDS, not this launch's size: a later handle of the same process may need more (run-time hop lengths).
 * Devices beyond the table opt in on every launch.  (The shim launches from one thread per GPU: setting a flag twice is harmless, a torn one is not possible.) */
inline void opt_in_big_lds(const void* fn, size_t lds, std::atomic<bool>* done_for_device) {
    if (lds <= 64 * 1024) return;
    int dev = 0;
    (void)hipGetDevice(&dev);
    const bool tracked = dev >= 0 && dev < BIG_LDS_DEVICES;
    if (tracked && done_for_device[dev].load(std::memory_order_acquire)) return;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, CU_LDS_BYTES) == hipSuccess && tracked) done_for_device[dev].store(true, std::memory_order_release);
}

}  // namespace

}  // namespace airband
#endif
