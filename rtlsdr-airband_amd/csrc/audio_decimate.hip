/* csrc/audio_decimate.hip -- output decimation by 2 (airband_hip_set_output_decimation / _decimate_audio): on a decimating handle this kernel stands in
 * audio_pack.hip's place.  A listed row of B float samples becomes B / 2 encoded samples: the encoder's float step (audio_sample.h, audio_q), the 47-tap integer
 * half-band FIR of audio_decimate.h over the channel's 46 carried q values followed by the row's, every second output kept, then little-endian int16 or G.711 and
 * the 16-byte record, computed on the outputs.  The definition is include/airband_hip.h's ("output decimation"); capi.audio_decimate_reference() is the same in
 * numpy.  One float32 multiplication per sample (compiled with -ffp-contract=off), integers behind it: the bytes are checked as bytes.
 *
 * It keeps audio_pack.hip's shape: a fixed grid, ONE wavefront per workgroup that owns a row at a time and strides over the rows; count and list read on the
 * device; the SOURCE rows read from out_wave with non-temporal 16-byte loads; every index clamped to its buffer.
 *
 * A row in LDS.  The stream S = history (46) followed by q(row) (B) is stored deinterleaved, S[2 m] in `even` and S[2 m + 1] in `odd`, because the half-band's
 * non-zero taps lie on ONE parity: output n is 24 multiply-adds over even[n .. n + 23] plus 16384 * odd[n + 11].  A lane makes four consecutive outputs from
 * fourteen dwords of `even` (pairs of int16 against pairs of taps) and two of `odd`: audio_decimate_four().  (B + 48) int16: 4 KiB at B = 2 000.
 * `odd` is stored one slot late, so that the four centre samples of a lane's outputs are one aligned 8-byte read and a lane's two odd q values one dword store.
 *
 * History.  Channel c's 46 values are 23 dwords at hist + 46 c, (S[2 l], S[2 l + 1]) in dword l = (even[l], odd[l]): lanes 0 .. 22 load them into LDS in front of
 * the row and, after the wavefront has met (the old values are in LDS by then: the new ones are written after the last read of the old), store (even, odd)[B / 2 + l]
 * back.  "A channel not listed in a step restarts from zeros" is a stamp: stamp[c] is the last step that listed c, and a history whose stamp is not k - 1 reads as
 * zeros.  No pass over the channels that are NOT listed: they are most of a fleet.
 * hist and stamp ASSUME THAT THE LIST'S ENTRIES ARE UNIQUE (the gate's list is ascending, airband_hip_decimate_audio's rows are their own channels): a row's
 * wavefront reads and writes its channel's 23 dwords and stamp without ordering against any other.  Only a damaged list, whose out-of-range entry is clamped onto
 * a channel that is also listed, has two wavefronts on one history: the buffers stay in bounds, that channel's audio is then undefined for the step.
 */
#include <hip/hip_runtime.h>

#include "audio_decimate.h"
#include "audio_sample.h" /* audio_q, audio_ulaw, audio_alaw: shared with audio_pack.hip and mixer_gate.hip */
#include "common.h"
#include "kernels.h"
#include "wave_lds.h"

namespace airband {

namespace {
typedef float ad_v4f __attribute__((ext_vector_type(4)));
typedef unsigned ad_v2u __attribute__((ext_vector_type(2)));
typedef unsigned ad_v4u __attribute__((ext_vector_type(4)));
constexpr int AUDIO_DECIMATE_MAX_GRID = 8192; /* 256 CUs x 32 wavefronts */
constexpr int AD_HIST_DWORDS = AUDIO_DECIMATE_HIST / 2;

template <int ENC>
__device__ __forceinline__ void audio_decimate_rows(const AudioDecimateArgs& a) {
    AB_DYNAMIC_LDS_BYTES(lds);
    const int lane = threadIdx.x & 63;
    int n = a.count ? a.count[0] : a.n_rows;
    n = n < a.max_rows ? n : a.max_rows;
    const int B = a.wave_batch, Bo = B / 2, nvec = B / 4, nout = B / 8;
    short* const even = reinterpret_cast<short*>(lds);  /* even[m] = S[2 m], m < Bo + 23; one slot of padding */
    short* const odd = even + Bo + 24;                   /* odd[m + 1] = S[2 m + 1] */
    const short* const centre = odd + 12;                /* centre[n] = S[2 n + 23] */
    for (int r = blockIdx.x; r < n; r += gridDim.x) {
        const int c = a.index ? a.index[r] : r;
        const int src_row = c < 0 ? 0 : (c < a.n_ch ? c : a.n_ch - 1);
        const ad_v4f* src = reinterpret_cast<const ad_v4f*>(a.src + (long)src_row * a.src_stride + a.src_pad);
        unsigned* const hist = a.hist ? reinterpret_cast<unsigned*>(a.hist) + (long)src_row * AD_HIST_DWORDS : nullptr;
        const bool carried = hist && (!a.stamp || a.stamp[src_row] == a.k - 1u);
        AB_WAVE_SYNC(); /* every lane is done with the row before */
        if (lane < AD_HIST_DWORDS) {
            const unsigned g = carried ? hist[lane] : 0u;
            even[lane] = (short)(g & 0xFFFFu);
            odd[lane + 1] = (short)(g >> 16);
        } else if (lane == AD_HIST_DWORDS) {
            even[Bo + 23] = 0; /* the padding: read with the last pair of even[] and not used */
            if (a.stamp) a.stamp[src_row] = a.k;
        }
        int peak = 0, n_clipped = 0, first = Bo, end = 0;
        /* four passes at a time: their loads are in flight together, as in audio_pack_rows */
        for (int u0 = lane; u0 < nvec; u0 += 4 * 64) {
            ad_v4f xs[4] = {};
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (u0 + 64 * i < nvec) xs[i] = __builtin_nontemporal_load(src + u0 + 64 * i);
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int u = u0 + 64 * i;
                if (u < nvec) {
                    const int q0 = audio_q(xs[i].x, n_clipped), q1 = audio_q(xs[i].y, n_clipped), q2 = audio_q(xs[i].z, n_clipped), q3 = audio_q(xs[i].w, n_clipped);
                    even[23 + 2 * u] = (short)q0;
                    even[24 + 2 * u] = (short)q2;
                    *reinterpret_cast<unsigned*>(odd + 24 + 2 * u) = ((unsigned)q1 & 0xFFFFu) | ((unsigned)q3 << 16);
                }
            }
        }
        AB_WAVE_SYNC(); /* S is whole */
        if (hist && lane < AD_HIST_DWORDS) hist[lane] = ((unsigned)(unsigned short)even[Bo + lane]) | ((unsigned)(unsigned short)odd[Bo + lane + 1] << 16);
        uint8_t* const dst = static_cast<uint8_t*>(a.audio) + (long)r * Bo * (ENC == AIRBAND_AUDIO_S16 ? 2 : 1);
        for (int v = lane; v < nout; v += 64) { /* a lane's indices ascend */
            int y[4];
            audio_decimate_four(even, centre, v, y, n_clipped);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int mag = y[j] < 0 ? -y[j] : y[j];
                peak = mag > peak ? mag : peak;
                if (y[j] != 0) {
                    const int i = 4 * v + j;
                    first = i < first ? i : first;
                    end = i + 1;
                }
            }
            if (ENC == AIRBAND_AUDIO_S16) {
                ad_v2u o;
                o.x = ((unsigned)y[0] & 0xFFFFu) | ((unsigned)y[1] << 16);
                o.y = ((unsigned)y[2] & 0xFFFFu) | ((unsigned)y[3] << 16);
                __builtin_nontemporal_store(o, reinterpret_cast<ad_v2u*>(dst) + v);
            } else {
                unsigned o;
                if (ENC == AIRBAND_AUDIO_ULAW)
                    o = audio_ulaw(y[0]) | (audio_ulaw(y[1]) << 8) | (audio_ulaw(y[2]) << 16) | (audio_ulaw(y[3]) << 24);
                else
                    o = audio_alaw(y[0]) | (audio_alaw(y[1]) << 8) | (audio_alaw(y[2]) << 16) | (audio_alaw(y[3]) << 24);
                __builtin_nontemporal_store(o, reinterpret_cast<unsigned*>(dst) + v);
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
            ad_v4u rec;
            rec.x = (unsigned)c;
            rec.y = (unsigned)peak | ((unsigned)n_clipped << 16);
            rec.z = (unsigned)first | ((unsigned)end << 16);
            rec.w = 0u;
            *reinterpret_cast<ad_v4u*>(a.info + r) = rec;
        }
    }
}
}  // namespace

__global__ __launch_bounds__(64) void audio_decimate_s16_kernel(AudioDecimateArgs a) { audio_decimate_rows<AIRBAND_AUDIO_S16>(a); }
__global__ __launch_bounds__(64) void audio_decimate_ulaw_kernel(AudioDecimateArgs a) { audio_decimate_rows<AIRBAND_AUDIO_ULAW>(a); }
__global__ __launch_bounds__(64) void audio_decimate_alaw_kernel(AudioDecimateArgs a) { audio_decimate_rows<AIRBAND_AUDIO_ALAW>(a); }

size_t audio_decimate_lds_bytes(int wave_batch) { return ((size_t)wave_batch + 48) * sizeof(short); }

void launch_audio_decimate(const AudioDecimateArgs& a, int grid, hipStream_t stream) {
    int gx = grid > 0 ? grid : (a.max_rows < AUDIO_DECIMATE_MAX_GRID ? a.max_rows : AUDIO_DECIMATE_MAX_GRID);
    if (gx < 1) return;
    const size_t lds = audio_decimate_lds_bytes(a.wave_batch);
    if (a.encoding == AIRBAND_AUDIO_S16)
        hipLaunchKernelGGL(audio_decimate_s16_kernel, dim3(gx), dim3(64), lds, stream, a);
    else if (a.encoding == AIRBAND_AUDIO_ULAW)
        hipLaunchKernelGGL(audio_decimate_ulaw_kernel, dim3(gx), dim3(64), lds, stream, a);
    else if (a.encoding == AIRBAND_AUDIO_ALAW)
        hipLaunchKernelGGL(audio_decimate_alaw_kernel, dim3(gx), dim3(64), lds, stream, a);
}

}  // namespace airband
