/* csrc/band_pack.h -- the rows' 16-byte records of one batch packed into one fleet-wide list in row order: the second kernel of the band watch (its events) and of
 * the band follow (its changes).
 *
 * ONE workgroup of sixteen wavefronts walks the rows in chunks of 1 024 with a carried total: an exclusive prefix sum of the rows' counts (shuffles inside a
 * wavefront, sixteen totals through LDS in two alternating sets: one barrier a chunk), then thread t copies its row's records from the row's staging slice to
 * list[offset ..) while below max_list, 16 bytes a record.  65 536 rows are 64 chunks of a load, six shuffles and a barrier each, and a batch has records on a
 * few rows: a single workgroup is enough at that size, and the order cannot depend on which workgroup arrives first because there is only one.  A row's count is
 * clamped to its slice before anything is indexed with it.
 */
#ifndef AIRBAND_CSRC_BAND_PACK_H
#define AIRBAND_CSRC_BAND_PACK_H

#include <hip/hip_runtime.h>

namespace airband {

constexpr int PACK_THREADS = 1024, PACK_WAVES = PACK_THREADS / 64;

/* counts[row * count_pitch]: the row's records, at stage[row * cap ..); called by every thread of a workgroup of PACK_THREADS */
__device__ __forceinline__ void pack_rows(const int* counts, int count_pitch, const uint4* stage, int cap, uint4* list, int max_list, int* n_list, int n_rows) {
    __shared__ int wave_total[2][PACK_WAVES];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = 0; /* the records of the rows in front of the chunk: the same in every thread */
    int chunk = 0;
#pragma unroll 1
    for (int r0 = 0; r0 < n_rows; r0 += PACK_THREADS, chunk++) {
        const int row = r0 + tid;
        int n = row < n_rows ? counts[(long)row * count_pitch] : 0;
        n = n < 0 ? 0 : n;
        n = n > cap ? cap : n;
        int incl = n;
#pragma unroll
        for (int dl = 1; dl < 64; dl <<= 1) {
            const int o = (int)__shfl_up((unsigned)incl, (unsigned)dl);
            if (lane >= dl) incl += o;
        }
        int* const tot = wave_total[chunk & 1]; /* written again two chunks on: every thread has passed the barrier between */
        if (lane == 63) tot[wave] = incl;
        __syncthreads();
        int before = carry, all = 0;
        for (int w = 0; w < PACK_WAVES; w++) {
            const int v = tot[w];
            before += w < wave ? v : 0;
            all += v;
        }
        const long off = (long)before + (incl - n);
        const uint4* const src = stage + (long)row * cap;
        for (int i = 0; i < n && off + i < (long)max_list; i++) list[off + i] = src[i];
        carry += all;
    }
    if (tid == 0) n_list[0] = carry;
}

}  // namespace airband
#endif
