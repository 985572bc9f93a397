/* csrc/audio_pack.hip -- encoded audio collect (airband_hip_set_output_encoding / _collect_active_encoded / _encode_audio): the rows the output gate delivers as
 * little-endian int16 or G.711 bytes instead of float32, and one 16-byte record per row (peak, clipped samples, where the audio starts and ends).  The definition
 * is include/airband_hip.h's ("encoded audio collect"); capi.audio_encode_reference() is the same in numpy.  One float32 multiplication per sample (this file is
 * compiled with -ffp-contract=off: nothing may fuse it with the rounding behind it), everything after it is integer arithmetic, so the bytes are checked as bytes.
 *
 * One launch per batch on a handle with an encoding, behind gate_index_kernel on the same stream (driver_gate.cpp, launch_gate_behind_mix, called by run_back_half); none on a handle without one.
 * It reads the SOURCE rows the gather reads -- out_wave + channel * wave_stride + AB_OUT_PAD -- not the packed float rows: it does not wait for the gather, and
 * the two read the same lines within microseconds of each other.
 *
 * Grid and lanes.  How many rows there are is on the device, so the grid is fixed and workgroups stride over the rows as in gate_gather_kernel.  A workgroup is
 * ONE wavefront and owns a row at a time: the row record is a reduction over the lane's passes and then across the 64 lanes (shuffles; no LDS, no atomics).
 * A lane loads 16 bytes (four samples), converts them and stores 8 bytes (S16) or 4 bytes (G.711): 64 lanes read 1 KiB and write 512 or 256 contiguous bytes.
 * Both ends of a source row are 16-byte aligned (see gate.hip) and wave_batch is a multiple of four, so every packed row starts on a multiple of 8 (S16) or 4
 * (G.711) bytes.  Loads and stores are non-temporal: the source is read once here, the packed row is read next by a copy engine.
 *
 * Every index is clamped to its buffer: the row count to max_rows, a listed channel to n_ch.
 */
#include <hip/hip_runtime.h>

#include "audio_sample.h" /* audio_q, audio_ulaw, audio_alaw: shared with mixer_gate.hip */
#include "common.h"
#include "kernels.h"

namespace airband {

namespace {
typedef float ap_v4f __attribute__((ext_vector_type(4)));
typedef unsigned ap_v2u __attribute__((ext_vector_type(2)));
typedef unsigned ap_v4u __attribute__((ext_vector_type(4)));
constexpr int AUDIO_PACK_MAX_GRID = 8192; /* 256 CUs x 32 wavefronts */

/* samples 4 v .. 4 v + 3 of a row: converted, stored at `row` (the packed row's first byte) and entered into the lane's share of the record; a lane calls this with
 * ascending v */
template <int ENC>
__device__ __forceinline__ void audio_pack_four(ap_v4f x, int v, uint8_t* row, int& peak, int& n_clipped, int& first, int& end) {
    int q[4];
    q[0] = audio_q(x.x, n_clipped);
    q[1] = audio_q(x.y, n_clipped);
    q[2] = audio_q(x.z, n_clipped);
    q[3] = audio_q(x.w, n_clipped);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int mag = q[j] < 0 ? -q[j] : q[j];
        peak = mag > peak ? mag : peak;
        if (q[j] != 0) {
            const int i = 4 * v + j;
            first = i < first ? i : first;
            end = i + 1;
        }
    }
    if (ENC == AIRBAND_AUDIO_S16) {
        ap_v2u o;
        o.x = ((unsigned)q[0] & 0xFFFFu) | ((unsigned)q[1] << 16);
        o.y = ((unsigned)q[2] & 0xFFFFu) | ((unsigned)q[3] << 16);
        __builtin_nontemporal_store(o, reinterpret_cast<ap_v2u*>(row) + v);
    } else {
        unsigned o;
        if (ENC == AIRBAND_AUDIO_ULAW)
            o = audio_ulaw(q[0]) | (audio_ulaw(q[1]) << 8) | (audio_ulaw(q[2]) << 16) | (audio_ulaw(q[3]) << 24);
        else
            o = audio_alaw(q[0]) | (audio_alaw(q[1]) << 8) | (audio_alaw(q[2]) << 16) | (audio_alaw(q[3]) << 24);
        __builtin_nontemporal_store(o, reinterpret_cast<unsigned*>(row) + v);
    }
}

template <int ENC>
__device__ __forceinline__ void audio_pack_rows(const AudioPackArgs& a) {
    const int lane = threadIdx.x & 63;
    int n = a.count ? a.count[0] : a.n_rows;
    n = n < a.max_rows ? n : a.max_rows;
    const int B = a.wave_batch, nvec = B / 4;
    for (int r = blockIdx.x; r < n; r += gridDim.x) {
        const int c = a.index ? a.index[r] : r;
        const int src_row = c < 0 ? 0 : (c < a.n_ch ? c : a.n_ch - 1);
        const ap_v4f* src = reinterpret_cast<const ap_v4f*>(a.src + (long)src_row * a.src_stride + a.src_pad);
        uint8_t* const dst = static_cast<uint8_t*>(a.audio) + (long)r * B * (ENC == AIRBAND_AUDIO_S16 ? 2 : 1);
        int peak = 0, n_clipped = 0, first = B, end = 0;
        /* four passes at a time: their loads are in flight together (a row of 1 000 samples is one such round, of 2 000 two) */
        for (int v0 = lane; v0 < nvec; v0 += 4 * 64) {
            ap_v4f xs[4] = {};
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (v0 + 64 * u < nvec) xs[u] = __builtin_nontemporal_load(src + v0 + 64 * u);
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int v = v0 + 64 * u; /* a lane's indices ascend */
                if (v < nvec) audio_pack_four<ENC>(xs[u], v, dst, peak, n_clipped, first, end);
            }
        }
        /* the row's record: every lane of the wavefront is here (n and the row loop are wave-uniform) */
        for (int d = 32; d >= 1; d >>= 1) {
            const int op = __shfl_xor(peak, d), of = __shfl_xor(first, d), oe = __shfl_xor(end, d);
            n_clipped += __shfl_xor(n_clipped, d);
            peak = op > peak ? op : peak;
            first = of < first ? of : first;
            end = oe > end ? oe : end;
        }
        if (lane == 0) {
            ap_v4u rec;
            rec.x = (unsigned)c;
            rec.y = (unsigned)peak | ((unsigned)n_clipped << 16);
            rec.z = (unsigned)first | ((unsigned)end << 16);
            rec.w = 0u;
            *reinterpret_cast<ap_v4u*>(a.info + r) = rec;
        }
    }
}
}  // namespace

__global__ __launch_bounds__(64) void audio_pack_s16_kernel(AudioPackArgs a) { audio_pack_rows<AIRBAND_AUDIO_S16>(a); }
__global__ __launch_bounds__(64) void audio_pack_ulaw_kernel(AudioPackArgs a) { audio_pack_rows<AIRBAND_AUDIO_ULAW>(a); }
__global__ __launch_bounds__(64) void audio_pack_alaw_kernel(AudioPackArgs a) { audio_pack_rows<AIRBAND_AUDIO_ALAW>(a); }

void launch_audio_pack(const AudioPackArgs& a, int grid, hipStream_t stream) {
    int gx = grid > 0 ? grid : (a.max_rows < AUDIO_PACK_MAX_GRID ? a.max_rows : AUDIO_PACK_MAX_GRID);
    if (gx < 1) return;
    if (a.encoding == AIRBAND_AUDIO_S16)
        hipLaunchKernelGGL(audio_pack_s16_kernel, dim3(gx), dim3(64), 0, stream, a);
    else if (a.encoding == AIRBAND_AUDIO_ULAW)
        hipLaunchKernelGGL(audio_pack_ulaw_kernel, dim3(gx), dim3(64), 0, stream, a);
    else if (a.encoding == AIRBAND_AUDIO_ALAW)
        hipLaunchKernelGGL(audio_pack_alaw_kernel, dim3(gx), dim3(64), 0, stream, a);
}

}  // namespace airband
