/* csrc/gate.hip -- signal-gated collect (airband_hip_set_output_gate / _collect_active): which channels' result rows a batch delivers, and those rows packed
 * into one dense buffer so that the host copies what it will use instead of every channel's row.
 *
 * The rule is the reference's file-output rule (src/output.cpp:501,531): a non-continuous sink writes a batch iff the channel has signal in it or had signal in the
 * batch before (`active`), so the one batch a transmission ended in still goes out whole.  `prev` is that `active`, kept per channel on the device and advanced
 * once per batch by the select pass -- it follows the batches in the order stage 2 ran them, whatever enqueued them.
 *
 * Three launches per batch on a gated handle, behind the emit / mixer launches (driver_gate.cpp, launch_gate_behind_mix, called by run_back_half); none on a handle without a gate:
 *   gate_select_kernel   one lane per channel: the verdict, the new `prev`, one 64-bit ballot per wavefront, one count per workgroup;
 *   gate_index_kernel    the same lanes again: workgroup base = sum of the counts in front of it, lane rank = population count of the ballot's lower bits ->
 *                        the list of active channels in ASCENDING order whatever the workgroups' scheduling (no atomic cursor), and the total;
 *   gate_gather_kernel   row i of the packed buffers = the row of channel index[i], 16 bytes per lane.
 */
#include <hip/hip_runtime.h>

#include "common.h"
#include "gate_passes.h"
#include "kernels.h"

namespace airband {

namespace {
typedef float v4f __attribute__((ext_vector_type(4)));
}  // namespace

/* (the two passes themselves are gate_passes.h's, shared with the mixer gate: here the verdict is the channel rule) */
__global__ __launch_bounds__(GATE_BLOCK) void gate_select_kernel(GateArgs a) {
    const int c = blockIdx.x * GATE_BLOCK + threadIdx.x;
    bool active = false;
    if (c < a.n_ch) {
        const unsigned g = a.gate[c];
        const bool on = !(g & AB_GATE_OFF);          /* a switched-off dongle delivers nothing and forgets its last batch (disable_device_outputs()) */
        const bool signal = on && a.axc[c] != ' ';   /* '*', and AFC's '<' / '>' */
        const unsigned kind = g & 3u;
        active = on && (kind == AIRBAND_GATE_ALWAYS || (kind == AIRBAND_GATE_SIGNAL && (signal || a.prev[c] != 0)));
        a.prev[c] = signal ? 1 : 0;
    }
    gate_select_pass(active, c, a.n_ch, a.mask, a.block_count);
}

__global__ __launch_bounds__(GATE_BLOCK) void gate_index_kernel(GateArgs a) {
    gate_index_pass(blockIdx.x * GATE_BLOCK + threadIdx.x, a.n_ch, a.mask, a.block_count, a.index, a.count, a.max_rows);
}

/* blockIdx.y 0: the audio rows, 1: the raw-I/Q rows.  A workgroup takes rows blockIdx.x, blockIdx.x + gridDim.x, ...: the grid does not depend on the count, which
 * only the device knows.  Both ends of a row are 16-byte aligned (AB_OUT_PAD = 28 floats in front of a 128-byte-pitched row; WAVE_BATCH is a multiple of four), and
 * eight consecutive lanes move one 128-byte line.  The source is read once and the packed row is read next by a copy engine, not by a CU: non-temporal both ways
 * (the load passes L1 by, the store does not claim a place in it). */
__global__ __launch_bounds__(256) void gate_gather_kernel(GateArgs a) {
    const int n = a.count[0] < a.max_rows ? a.count[0] : a.max_rows;
    const bool iq = blockIdx.y == 1;
    const int row_floats = iq ? 2 * a.wave_batch : a.wave_batch, nvec = row_floats / 4;
    for (int r = blockIdx.x; r < n; r += gridDim.x) {
        const int c = a.index[r];
        const float* src = iq ? a.out_iq + (long)c * row_floats : a.out_wave + (long)c * a.wave_stride + AB_OUT_PAD;
        float* dst = (iq ? a.iq_rows : a.rows) + (long)r * row_floats;
        for (int v = threadIdx.x; v < nvec; v += 256)
            __builtin_nontemporal_store(__builtin_nontemporal_load(reinterpret_cast<const v4f*>(src) + v), reinterpret_cast<v4f*>(dst) + v);
    }
}

int gate_blocks(int n_ch) { return (n_ch + GATE_BLOCK - 1) / GATE_BLOCK; }

void launch_gate(const GateArgs& a, hipStream_t stream) {
    const int nb = gate_blocks(a.n_ch);
    hipLaunchKernelGGL(gate_select_kernel, dim3(nb), dim3(GATE_BLOCK), 0, stream, a);
    hipLaunchKernelGGL(gate_index_kernel, dim3(nb), dim3(GATE_BLOCK), 0, stream, a);
    /* eight workgroups of four wavefronts fill a CU; 256 CUs */
    const int gx = a.max_rows < 2048 ? a.max_rows : 2048;
    hipLaunchKernelGGL(gate_gather_kernel, dim3(gx, a.iq_rows ? 2 : 1), dim3(256), 0, stream, a);
}

}  // namespace airband
