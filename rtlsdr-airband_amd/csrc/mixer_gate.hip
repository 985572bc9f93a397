/* csrc/mixer_gate.hip -- gated mixer collect (airband_hip_set_mixer_gate / _mixer_gate_step / _collect_active_mixers / _encode_mixer_audio): which mixers' sums a
 * step delivers, and those rows packed into one dense buffer as float32, int16 or G.711 frames with one 16-byte record per row.  The definition is
 * include/airband_hip.h's ("gated mixer collect"); capi.mixer_gate_reference() is the same in numpy.  The rule is the channel gate's (gate.hip) with the mixer's
 * has_signal in the place of axcindicate; the samples are the encoder's (audio_sample.h): one float32 multiplication per sample (this file is compiled with
 * -ffp-contract=off), everything after it is integer arithmetic, so the bytes are checked as bytes.
 *
 * Three launches per step on a handle with a mixer gate (driver_mix.cpp, launch_mixer_gate_step: behind the batch's mixer sums in run_back_half, or where
 * airband_hip_mixer_gate_step() puts it); none on a handle without one:
 *   mixer_gate_select_kernel   one lane per mixer: the verdict, the new `prev`, then gate_passes.h's ballot and workgroup count;
 *   mixer_gate_index_kernel    gate_passes.h's rank pass: the ascending list and the total;
 *   mixer_pack_*_kernel        row i of the packed buffer = the frames of mixer index[i], and its record.
 *
 * Pack: grid and lanes.  How many rows there are is on the device, so the grid is fixed and workgroups stride over the rows.  A workgroup is ONE wavefront and
 * owns a row at a time: the record is a reduction over the lane's passes and then across the 64 lanes (shuffles; no LDS, no atomics).  A lane takes four frames
 * per pass: 16 bytes of `left` (and 16 of `right` when the rows are stereo), and stores them interleaved L, R: 16 / 32 bytes as float32, 8 / 16 as int16, 4 / 8 as
 * G.711.  Rows of left / right are wave_batch floats apart in hipMalloc'ed buffers and wave_batch is a multiple of four: every load is 16-byte aligned, and every
 * packed row starts on a multiple of its lane's store.  Loads and stores are non-temporal: the sums are read once here, the packed row is read next by a copy
 * engine.
 *
 * Every index is clamped to its buffer: the row count to max_rows, a listed mixer to n_mixers.
 */
#include <hip/hip_runtime.h>

#include "audio_sample.h"
#include "common.h"
#include "gate_passes.h"
#include "kernels.h"

namespace airband {

namespace {
typedef float mg_v4f __attribute__((ext_vector_type(4)));
typedef unsigned mg_v2u __attribute__((ext_vector_type(2)));
typedef unsigned mg_v4u __attribute__((ext_vector_type(4)));
constexpr int MIXER_PACK_MAX_GRID = 8192; /* 256 CUs x 32 wavefronts */

template <int ENC>
__device__ __forceinline__ unsigned mixer_law(int q) {
    return ENC == AIRBAND_AUDIO_ULAW ? audio_ulaw(q) : audio_alaw(q);
}

/* frames 4 v .. 4 v + 3 of a row: converted, stored at `row` (the packed row's first byte) and entered into the lane's share of the record; a lane calls this
 * with ascending v.  W == 1: r is not looked at. */
template <int ENC, int W>
__device__ __forceinline__ void mixer_pack_four(mg_v4f l, mg_v4f r, int v, uint8_t* row, int& peak, int& n_clipped, int& first, int& end) {
    if (ENC == AIRBAND_AUDIO_F32) { /* the bits of the sums */
        if (W == 1) {
            __builtin_nontemporal_store(l, reinterpret_cast<mg_v4f*>(row) + v);
        } else {
            const mg_v4f o0 = {l.x, r.x, l.y, r.y}, o1 = {l.z, r.z, l.w, r.w};
            __builtin_nontemporal_store(o0, reinterpret_cast<mg_v4f*>(row) + 2 * v);
            __builtin_nontemporal_store(o1, reinterpret_cast<mg_v4f*>(row) + 2 * v + 1);
        }
        return;
    }
    int ql[4], qr[4] = {0, 0, 0, 0};
    ql[0] = audio_q(l.x, n_clipped);
    ql[1] = audio_q(l.y, n_clipped);
    ql[2] = audio_q(l.z, n_clipped);
    ql[3] = audio_q(l.w, n_clipped);
    if (W == 2) {
        qr[0] = audio_q(r.x, n_clipped);
        qr[1] = audio_q(r.y, n_clipped);
        qr[2] = audio_q(r.z, n_clipped);
        qr[3] = audio_q(r.w, n_clipped);
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int ml = ql[j] < 0 ? -ql[j] : ql[j], mr = qr[j] < 0 ? -qr[j] : qr[j];
        const int mag = ml > mr ? ml : mr;
        peak = mag > peak ? mag : peak;
        if (mag != 0) { /* the FRAME has audio */
            const int i = 4 * v + j;
            first = i < first ? i : first;
            end = i + 1;
        }
    }
    if (ENC == AIRBAND_AUDIO_S16) {
        if (W == 1) {
            mg_v2u o;
            o.x = ((unsigned)ql[0] & 0xFFFFu) | ((unsigned)ql[1] << 16);
            o.y = ((unsigned)ql[2] & 0xFFFFu) | ((unsigned)ql[3] << 16);
            __builtin_nontemporal_store(o, reinterpret_cast<mg_v2u*>(row) + v);
        } else {
            mg_v4u o;
            o.x = ((unsigned)ql[0] & 0xFFFFu) | ((unsigned)qr[0] << 16);
            o.y = ((unsigned)ql[1] & 0xFFFFu) | ((unsigned)qr[1] << 16);
            o.z = ((unsigned)ql[2] & 0xFFFFu) | ((unsigned)qr[2] << 16);
            o.w = ((unsigned)ql[3] & 0xFFFFu) | ((unsigned)qr[3] << 16);
            __builtin_nontemporal_store(o, reinterpret_cast<mg_v4u*>(row) + v);
        }
    } else if (W == 1) {
        const unsigned o = mixer_law<ENC>(ql[0]) | (mixer_law<ENC>(ql[1]) << 8) | (mixer_law<ENC>(ql[2]) << 16) | (mixer_law<ENC>(ql[3]) << 24);
        __builtin_nontemporal_store(o, reinterpret_cast<unsigned*>(row) + v);
    } else {
        mg_v2u o;
        o.x = mixer_law<ENC>(ql[0]) | (mixer_law<ENC>(qr[0]) << 8) | (mixer_law<ENC>(ql[1]) << 16) | (mixer_law<ENC>(qr[1]) << 24);
        o.y = mixer_law<ENC>(ql[2]) | (mixer_law<ENC>(qr[2]) << 8) | (mixer_law<ENC>(ql[3]) << 16) | (mixer_law<ENC>(qr[3]) << 24);
        __builtin_nontemporal_store(o, reinterpret_cast<mg_v2u*>(row) + v);
    }
}

template <int ENC, int W>
__device__ __forceinline__ void mixer_pack_rows(const MixerPackArgs& a) {
    const int lane = threadIdx.x & 63;
    int n = a.count ? a.count[0] : a.n_rows;
    n = n < a.max_rows ? n : a.max_rows;
    const int B = a.wave_batch, nvec = B / 4;
    constexpr int SAMPLE_BYTES = ENC == AIRBAND_AUDIO_F32 ? 4 : (ENC == AIRBAND_AUDIO_S16 ? 2 : 1);
    for (int r = blockIdx.x; r < n; r += gridDim.x) {
        const int m = a.index ? a.index[r] : r;
        const int src_row = m < 0 ? 0 : (m < a.n_mixers ? m : a.n_mixers - 1);
        const mg_v4f* left = reinterpret_cast<const mg_v4f*>(a.left + (long)src_row * B);
        const mg_v4f* right = W == 2 ? reinterpret_cast<const mg_v4f*>(a.right + (long)src_row * B) : left; /* mono: a.right may be null, and is not read */
        uint8_t* const dst = static_cast<uint8_t*>(a.out) + (long)r * B * (W * SAMPLE_BYTES);
        int peak = 0, n_clipped = 0, first = B, end = 0;
        /* four passes at a time: their loads are in flight together (a row of 1 000 frames is one such round, of 2 000 two) */
        for (int v0 = lane; v0 < nvec; v0 += 4 * 64) {
            mg_v4f xl[4] = {}, xr[4] = {};
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (v0 + 64 * u < nvec) {
                    xl[u] = __builtin_nontemporal_load(left + v0 + 64 * u);
                    if (W == 2) xr[u] = __builtin_nontemporal_load(right + v0 + 64 * u);
                }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int v = v0 + 64 * u; /* a lane's indices ascend */
                if (v < nvec) mixer_pack_four<ENC, W>(xl[u], xr[u], v, dst, peak, n_clipped, first, end);
            }
        }
        if (ENC == AIRBAND_AUDIO_F32) continue; /* float rows carry no record */
        /* the row's record: every lane of the wavefront is here (n and the row loop are wave-uniform) */
        for (int d = 32; d >= 1; d >>= 1) {
            const int op = __shfl_xor(peak, d), of = __shfl_xor(first, d), oe = __shfl_xor(end, d);
            n_clipped += __shfl_xor(n_clipped, d);
            peak = op > peak ? op : peak;
            first = of < first ? of : first;
            end = oe > end ? oe : end;
        }
        if (lane == 0) {
            mg_v4u rec;
            rec.x = (unsigned)m;
            rec.y = (unsigned)peak | ((unsigned)n_clipped << 16); /* at most 2 * 2 000 clipped samples: it fits */
            rec.z = (unsigned)first | ((unsigned)end << 16);
            rec.w = a.stereo ? (a.stereo[src_row] != 0 ? 1u : 0u) : a.reserved_all;
            *reinterpret_cast<mg_v4u*>(a.info + r) = rec;
        }
    }
}
}  // namespace

__global__ __launch_bounds__(GATE_BLOCK) void mixer_gate_select_kernel(MixerGateArgs a) {
    const int m = blockIdx.x * GATE_BLOCK + threadIdx.x;
    bool active = false;
    if (m < a.n_mixers) {
        const unsigned g = a.gate[m];
        const bool signal = a.has_signal[m] != 0;
        active = g == AIRBAND_GATE_ALWAYS || (g == AIRBAND_GATE_SIGNAL && (signal || a.prev[m] != 0));
        a.prev[m] = signal ? 1 : 0;
    }
    gate_select_pass(active, m, a.n_mixers, a.mask, a.block_count);
}

__global__ __launch_bounds__(GATE_BLOCK) void mixer_gate_index_kernel(MixerGateArgs a) {
    gate_index_pass(blockIdx.x * GATE_BLOCK + threadIdx.x, a.n_mixers, a.mask, a.block_count, a.index, a.count, a.max_rows);
}

__global__ __launch_bounds__(64) void mixer_pack_f32_mono_kernel(MixerPackArgs a) { mixer_pack_rows<AIRBAND_AUDIO_F32, 1>(a); }
__global__ __launch_bounds__(64) void mixer_pack_f32_stereo_kernel(MixerPackArgs a) { mixer_pack_rows<AIRBAND_AUDIO_F32, 2>(a); }
__global__ __launch_bounds__(64) void mixer_pack_s16_mono_kernel(MixerPackArgs a) { mixer_pack_rows<AIRBAND_AUDIO_S16, 1>(a); }
__global__ __launch_bounds__(64) void mixer_pack_s16_stereo_kernel(MixerPackArgs a) { mixer_pack_rows<AIRBAND_AUDIO_S16, 2>(a); }
__global__ __launch_bounds__(64) void mixer_pack_ulaw_mono_kernel(MixerPackArgs a) { mixer_pack_rows<AIRBAND_AUDIO_ULAW, 1>(a); }
__global__ __launch_bounds__(64) void mixer_pack_ulaw_stereo_kernel(MixerPackArgs a) { mixer_pack_rows<AIRBAND_AUDIO_ULAW, 2>(a); }
__global__ __launch_bounds__(64) void mixer_pack_alaw_mono_kernel(MixerPackArgs a) { mixer_pack_rows<AIRBAND_AUDIO_ALAW, 1>(a); }
__global__ __launch_bounds__(64) void mixer_pack_alaw_stereo_kernel(MixerPackArgs a) { mixer_pack_rows<AIRBAND_AUDIO_ALAW, 2>(a); }

void launch_mixer_gate_list(const MixerGateArgs& a, hipStream_t stream) {
    const int nb = (a.n_mixers + GATE_BLOCK - 1) / GATE_BLOCK; /* gate_blocks(n_mixers) */
    hipLaunchKernelGGL(mixer_gate_select_kernel, dim3(nb), dim3(GATE_BLOCK), 0, stream, a);
    hipLaunchKernelGGL(mixer_gate_index_kernel, dim3(nb), dim3(GATE_BLOCK), 0, stream, a);
}

void launch_mixer_pack(const MixerPackArgs& a, int grid, hipStream_t stream) {
    const int gx = grid > 0 ? grid : (a.max_rows < MIXER_PACK_MAX_GRID ? a.max_rows : MIXER_PACK_MAX_GRID);
    if (gx < 1) return;
    const bool st = a.width == 2;
    if (a.encoding == AIRBAND_AUDIO_F32) {
        if (st) hipLaunchKernelGGL(mixer_pack_f32_stereo_kernel, dim3(gx), dim3(64), 0, stream, a);
        else hipLaunchKernelGGL(mixer_pack_f32_mono_kernel, dim3(gx), dim3(64), 0, stream, a);
    } else if (a.encoding == AIRBAND_AUDIO_S16) {
        if (st) hipLaunchKernelGGL(mixer_pack_s16_stereo_kernel, dim3(gx), dim3(64), 0, stream, a);
        else hipLaunchKernelGGL(mixer_pack_s16_mono_kernel, dim3(gx), dim3(64), 0, stream, a);
    } else if (a.encoding == AIRBAND_AUDIO_ULAW) {
        if (st) hipLaunchKernelGGL(mixer_pack_ulaw_stereo_kernel, dim3(gx), dim3(64), 0, stream, a);
        else hipLaunchKernelGGL(mixer_pack_ulaw_mono_kernel, dim3(gx), dim3(64), 0, stream, a);
    } else if (a.encoding == AIRBAND_AUDIO_ALAW) {
        if (st) hipLaunchKernelGGL(mixer_pack_alaw_stereo_kernel, dim3(gx), dim3(64), 0, stream, a);
        else hipLaunchKernelGGL(mixer_pack_alaw_mono_kernel, dim3(gx), dim3(64), 0, stream, a);
    }
}

}  // namespace airband
