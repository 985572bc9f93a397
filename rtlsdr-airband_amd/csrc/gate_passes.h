/* csrc/gate_passes.h -- the two list-building passes the gates share (gate.hip: channels; mixer_gate.hip: mixers): one lane per item, a verdict per lane, and from
 * the verdicts the ASCENDING list of the active items whatever the workgroups' scheduling -- no atomic cursor, so who is dropped past max_rows is defined.
 *   gate_select_pass   called by every lane of a GATE_BLOCK workgroup with its verdict: one 64-bit ballot per wavefront, one count per workgroup;
 *   gate_index_pass    the same lanes again, in a later launch: workgroup base = sum of the counts in front of it, lane rank = population count of the ballot's
 *                      lower bits -> the list, and the total.
 * What a verdict is -- the flag array, its "quiet" value, the memory of the batch before -- is the calling kernel's business. */
#pragma once

#include <hip/hip_runtime.h>

namespace airband {

constexpr int GATE_BLOCK = 1024; /* items (lanes) per workgroup of the select / index passes: 524 288 channels are 512 counts to sum per workgroup */
constexpr int GATE_WAVES = GATE_BLOCK / 64;

/* item c = blockIdx.x * GATE_BLOCK + threadIdx.x of n; `active` is false for c >= n */
__device__ __forceinline__ void gate_select_pass(bool active, int c, int n, unsigned long long* mask, int* block_count) {
    __shared__ int wave_count[GATE_WAVES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long m = __ballot(active); /* 64 lanes: bit i = lane i */
    if (lane == 0) {
        if (c < n) mask[c >> 6] = m;
        wave_count[w] = __popcll(m);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int k = 0;
        for (int i = 0; i < GATE_WAVES; i++) k += wave_count[i];
        block_count[blockIdx.x] = k;
    }
}

__device__ __forceinline__ void gate_index_pass(int c, int n, const unsigned long long* mask, const int* block_count, int* index, int* count, int max_rows) {
    __shared__ int wave_count[GATE_WAVES];
    __shared__ int base;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (threadIdx.x == 0) base = 0;
    __syncthreads();
    int before = 0; /* active items of the workgroups in front of this one (integer sums: the order of the additions does not show) */
    for (int j = threadIdx.x; j < (int)blockIdx.x; j += GATE_BLOCK) before += block_count[j];
    if (before) atomicAdd(&base, before);
    const unsigned long long m = (c - lane) < n ? mask[c >> 6] : 0ull;
    if (lane == 0) wave_count[w] = __popcll(m);
    __syncthreads();
    int pos = base;
    for (int i = 0; i < w; i++) pos += wave_count[i];
    pos += __popcll(m & ((1ull << lane) - 1ull));
    if (((m >> lane) & 1ull) && pos < max_rows) index[pos] = c; /* past max_rows: counted, not listed */
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        int k = base;
        for (int i = 0; i < GATE_WAVES; i++) k += wave_count[i];
        count[0] = k;
    }
}

}  // namespace airband
