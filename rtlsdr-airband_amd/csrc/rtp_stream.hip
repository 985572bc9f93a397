/* csrc/rtp_stream.hip -- RTP packet stream (airband_hip_set_rtp_stream / _collect_rtp_packets / _collect_rtp_state): the encoded rows the output gate lists, cut
 * into complete RTP packets of a fixed frame length on the GPU (RFC 3550 header, RFC 3551 payload), the remainder of a row carried per channel from batch to
 * batch, one 16-byte record per packet, one count, and per-channel sender state.  The definition is include/airband_hip.h's ("RTP packet stream");
 * capi.rtp_stream_reference() is the same in plain Python.  Integers only: packets, records and state are checked as bytes.
 *
 * The kernels are written against "a mask, its per-workgroup counts and encoded rows" (RtpArgs::gate_mask, ::gate_count, ::enc_audio): the driver fills them from
 * the output gate and the encoder, or from the mixer gate and the mixer pack (driver_gate.cpp, rtp_args over a SpoolSource): the mixer RTP stream
 * (airband_hip_set_mixer_rtp_stream) runs these same kernels, "channel" being the mixer.
 *
 * Frames.  A frame is W = 1 << width_shift samples (W = 2: a stereo mixer gate's L, R), FB = W * sample_bytes bytes: 1, 2 or 4.  Everything that counts time --
 * B, F, a carry length, state.carry, ts_start, a packet's timestamp, packets = (carry + B) / F -- counts FRAMES; everything that moves bytes -- the row, the carry
 * buffer, the payload dwords, `length`, octets -- multiplies by FB.
 * wave_batch B and frame_samples F are multiples of 4 frames, so every carry length -- a multiple of gcd(B, F) below F -- is a multiple of 4 frames as well:
 * 4 * FB bytes, which is 1, 2 or 4 whole dwords.  For W = 2: a carry of 4n frames is 8n bytes (G.711) or 16n bytes (S16), a packet's payload F * 2 * sample_bytes
 * bytes with F = 4m is 8m or 16m, a row B * 2 * sample_bytes likewise, the channel's carry buffer starts at c * carry_cap * FB with carry_cap a multiple of 4,
 * and a slot's payload starts at byte 12 of a 16-byte aligned slot.  So a carry, a row, a payload and a slot's payload offset are whole dwords whatever the
 * frame size, and a dword never straddles two frames' samples of different packets.  ALL MOVES ARE WHOLE DWORDS, four-byte aligned at both ends.  The S16 byte
 * swap is per 16-bit half of a dword and so does not care whether the halves are two mono samples or L and R of one frame.
 *
 * Three launches per step on a handle with a stream, behind the encoder on the same stream (driver_gate.cpp, launch_gate_behind_mix; driver_mix.cpp,
 * launch_mixer_gate_step); none on a handle without.  The flush (airband_hip_mixer_rtp_flush) is the same three launches with NO mask and no counts
 * (gate_mask == gate_count == NULL): nobody is listed, every carrying channel emits its flush packet; no pass indexes with the null pointers:
 *   rtp_count_kernel   one lane per channel: the channel's rank in the gate's mask (its row, were the list endless), listed or not, and from its carry how many
 *                      packets the step gives it; a channel that is neither listed nor carrying stops talking here.  Per workgroup the sums of packets, channels
 *                      with work, lost rows and payload bytes;
 *   rtp_scan_kernel    the same lanes: prefix sums over channels (wavefront shuffles, the wavefronts' totals, the workgroups in front) give every channel its
 *                      first slot and its place in the work list -- (channel ascending, time ascending), no atomic cursor; the last workgroup's first
 *                      thread books the count and the counters;
 *   rtp_write_kernel   one wavefront per channel with work, the grid fixed and striding over the work list (how long it is is on the device): lanes move dwords
 *                      from the carry and the row into the slots, lanes j write packet j's header and record, then -- every lane having read what it needs of
 *                      the old carry -- the row's remainder becomes the new carry and lane 0 advances the channel's state.
 * A value one of these kernels reads from the control block or the plan is never written by the same kernel.  The row is read once here and the slots are read
 * next by a copy engine: non-temporal loads and stores, as in audio_pack.hip.
 *
 * Every count and index read from device memory is clamped to its buffer before anything is indexed with it: the carry length, the work count, a work item's
 * channel, row and first slot; a slot at or past max_packets is not written.
 */
#include <hip/hip_runtime.h>

#include "common.h"
#include "gate_passes.h" /* GATE_BLOCK, GATE_WAVES: the layout of the mask and the counts this file ranks with */
#include "kernels.h"

/* the point between "every lane has read the old carry" and "the new carry is written": lanes of ONE wavefront.  On the GPU the wavefront's own vector memory
 * operations have completed (vmcnt(0); expcnt and lgkmcnt left alone) and the compiler keeps the order; tests/hostshim_wave64 makes its fibers meet. */
#if defined(AB_LOCKSTEP)
#define RTP_CARRY_READ() AB_LOCKSTEP()
#else
#define RTP_CARRY_READ()                                        \
    do {                                                        \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  \
        __builtin_amdgcn_s_waitcnt(0x0F70);                     \
        __builtin_amdgcn_wave_barrier();                        \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  \
    } while (0)
#endif

namespace airband {

namespace {
typedef unsigned rtp_v4u __attribute__((ext_vector_type(4)));
constexpr int RTP_MAX_GRID = 8192; /* one-wavefront workgroups: 256 CUs x 32 wavefronts, audio_pack.hip's grid */

__device__ __forceinline__ int rtp_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

/* the carry a state record names, in frames, as the kernels use it: whole dwords, inside the channel's carry buffer */
__device__ __forceinline__ int rtp_carry(const RtpArgs& a, const airband_hip_rtp_state& st) { return rtp_clamp((int)(st.carry & ~3u), 0, a.carry_cap); }

/* sum over the workgroup's lanes, called by all of them: shuffles, then the wavefronts' totals through LDS.  SET: every call site its own LDS */
template <int SET>
__device__ __forceinline__ int rtp_block_sum(int v) {
    __shared__ int wave_total[GATE_WAVES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    if (lane == 0) wave_total[w] = v;
    __syncthreads();
    int n = 0;
    for (int i = 0; i < GATE_WAVES; i++) n += wave_total[i];
    return n;
}

/* exclusive prefix of v over the workgroup's lanes, called by all of them; *total: the workgroup's sum */
template <int SET>
__device__ __forceinline__ int rtp_block_prefix(int v, int* total) {
    __shared__ int wave_total[GATE_WAVES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int dl = 1; dl < 64; dl <<= 1) {
        const int o = __shfl_up(incl, (unsigned)dl);
        if (lane >= dl) incl += o;
    }
    if (lane == 63) wave_total[w] = incl;
    __syncthreads();
    int before = 0, all = 0;
    for (int i = 0; i < GATE_WAVES; i++) {
        before += i < w ? wave_total[i] : 0;
        all += wave_total[i];
    }
    *total = all;
    return before + incl - v;
}
}  // namespace

__global__ __launch_bounds__(GATE_BLOCK) void rtp_count_kernel(RtpArgs a) {
    __shared__ int wave_count[GATE_WAVES];
    __shared__ int base;
    const int c = blockIdx.x * GATE_BLOCK + threadIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    /* the channel's rank among the gate's verdicts (gate_index_pass's scheme): its row, had the list no end */
    if (threadIdx.x == 0) base = 0;
    __syncthreads();
    const bool masked = a.gate_mask != nullptr && a.gate_count != nullptr; /* uniform; false: the flush, nobody is listed and neither pointer is followed */
    int before = 0;
    if (masked)
        for (int j = threadIdx.x; j < (int)blockIdx.x; j += GATE_BLOCK) before += a.gate_count[j];
    if (before) atomicAdd(&base, before);
    const unsigned long long m = (masked && (c - lane) < a.n_ch) ? a.gate_mask[c >> 6] : 0ull;
    if (lane == 0) wave_count[w] = __popcll(m);
    __syncthreads();
    int pos = base;
    for (int i = 0; i < w; i++) pos += wave_count[i];
    pos += __popcll(m & ((1ull << lane) - 1ull));

    const int fb = a.sample_bytes << a.width_shift; /* bytes of a frame */
    int np = 0, row = -1, lost = 0, octets = 0;
    if (c < a.n_ch) {
        if (a.sources[c].stream) {
            const airband_hip_rtp_state st = a.state[c];
            const int cn = rtp_carry(a, st);
            const bool selected = (m >> lane) & 1ull;
            if (selected && pos < a.max_rows) {
                row = pos;
                np = (cn + a.wave_batch) / a.frame_samples;
                octets = np * a.frame_samples * fb;
            } else {
                lost = selected ? 1 : 0; /* selected by the rule, dropped past max_rows */
                if (cn > 0) {
                    np = 1; /* the flush packet */
                    octets = cn * fb;
                } else if (st.flags & 1u) {
                    a.state[c].flags = st.flags & ~1u; /* not listed, nothing carried: the talkspurt is over, nothing is emitted */
                }
            }
        }
        RtpPlan p;
        p.np = np;
        p.row = row;
        a.plan[c] = p;
    }
    const int s_packets = rtp_block_sum<0>(np), s_work = rtp_block_sum<1>(np > 0 ? 1 : 0), s_lost = rtp_block_sum<2>(lost), s_octets = rtp_block_sum<3>(octets);
    if (threadIdx.x == 0) {
        RtpBlock b;
        b.packets = s_packets;
        b.work = s_work;
        b.lost = s_lost;
        b.octets = s_octets;
        a.blocks[blockIdx.x] = b;
    }
}

__global__ __launch_bounds__(GATE_BLOCK) void rtp_scan_kernel(RtpArgs a) {
    __shared__ int base_packets, base_work;
    __shared__ unsigned long long all_lost, all_octets;
    const int c = blockIdx.x * GATE_BLOCK + threadIdx.x;
    const bool last = blockIdx.x == gridDim.x - 1;
    if (threadIdx.x == 0) {
        base_packets = base_work = 0;
        all_lost = all_octets = 0ull;
    }
    __syncthreads();
    /* the workgroups in front (integer sums: the order of the additions does not show); the last workgroup also sums what only the counters want */
    int bp = 0, bw = 0;
    for (int j = threadIdx.x; j < (int)blockIdx.x; j += GATE_BLOCK) {
        bp += a.blocks[j].packets;
        bw += a.blocks[j].work;
    }
    if (bp) atomicAdd(&base_packets, bp);
    if (bw) atomicAdd(&base_work, bw);
    if (last) {
        unsigned long long l = 0ull, o = 0ull;
        for (int j = threadIdx.x; j < (int)gridDim.x; j += GATE_BLOCK) {
            l += (unsigned long long)a.blocks[j].lost;
            o += (unsigned long long)a.blocks[j].octets;
        }
        if (l) atomicAdd(&all_lost, l);
        if (o) atomicAdd(&all_octets, o);
    }
    const RtpPlan p = c < a.n_ch ? a.plan[c] : RtpPlan{0, -1};
    int n_packets = 0, n_work = 0;
    const int first = rtp_block_prefix<0>(p.np, &n_packets); /* its __syncthreads also publishes the bases */
    const int rank = rtp_block_prefix<1>(p.np > 0 ? 1 : 0, &n_work);
    if (p.np > 0 && base_work + rank < a.n_ch) {
        RtpWork it;
        it.channel = c;
        it.first = base_packets + first;
        it.row = p.row;
        it.pad = 0;
        a.work[base_work + rank] = it;
    }
    if (last && threadIdx.x == 0) {
        RtpCtl& t = *a.ctl;
        const int total = base_packets + n_packets;
        t.n_packets = total;
        t.n_work = base_work + n_work;
        t.packets += (unsigned long long)total;
        t.dropped += (unsigned long long)(total > a.max_packets ? total - a.max_packets : 0);
        t.octets += all_octets;
        t.lost_rows += all_lost;
    }
}

/* SB: bytes per sample, 1 (G.711: the encoder's bytes as they are) or 2 (L16 is network order: the encoder's little-endian int16 byte-swapped, L and R each);
 * W: samples per frame.  FB = SB * W bytes per frame: B, F, cn, rem and the timestamps count frames, the dword counts (Bd, cd, per, rd) come from bytes */
template <int SB, int W>
__device__ __forceinline__ void rtp_write(const RtpArgs& a) {
    constexpr int FB = SB * W;
    const int lane = threadIdx.x & 63;
    const int n_work = rtp_clamp(a.ctl->n_work, 0, a.n_ch);
    const int B = a.wave_batch, F = a.frame_samples, Bd = B * FB / 4;
    for (int w = blockIdx.x; w < n_work; w += gridDim.x) { /* wave-uniform */
        const RtpWork it = a.work[w];
        const int c = rtp_clamp(it.channel, 0, a.n_ch - 1);
        const bool listed = it.row >= 0;
        const int row = rtp_clamp(it.row, 0, a.max_rows - 1), first = rtp_clamp(it.first, 0, a.max_packets); /* at max_packets: nothing of it is written */
        const airband_hip_rtp_state st = a.state[c];
        const airband_hip_rtp_source src = a.sources[c];
        const int cn = rtp_carry(a, st), cd = cn * FB / 4;
        const int np = listed ? (cn + B) / F : (cn > 0 ? 1 : 0);
        const int per = listed ? F * FB / 4 : cd; /* payload dwords of one packet */
        const int nd = np * per;
        const uint32_t ts_start = src.ts0 + a.k * (uint32_t)B - (uint32_t)cn;
        unsigned* const carry = reinterpret_cast<unsigned*>(a.carry + (long)c * a.carry_stride);
        const unsigned* const rowp = reinterpret_cast<const unsigned*>(a.enc_audio + (long)row * B * FB);
        /* the payloads: dword d of the carry followed by the row is dword o of packet j.  Four passes at a time, their loads in flight together */
        if (nd > 0) {
            int j = lane / per, o = lane - j * per;
            for (int d0 = lane; d0 < nd; d0 += 4 * 64) {
                unsigned x[4] = {};
                long at[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int d = d0 + 64 * u;
                    at[u] = -1;
                    if (d < nd && first + j < a.max_packets) {
                        at[u] = (long)(first + j) * a.slot_bytes + 12 + 4 * o;
                        x[u] = __builtin_nontemporal_load(d < cd ? carry + d : rowp + (d - cd));
                    }
                    o += 64;
                    while (o >= per) {
                        o -= per;
                        j++;
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    if (at[u] < 0) continue;
                    const unsigned v = SB == 2 ? (((x[u] & 0xFF00FF00u) >> 8) | ((x[u] & 0x00FF00FFu) << 8)) : x[u];
                    __builtin_nontemporal_store(v, reinterpret_cast<unsigned*>(a.packets + at[u]));
                }
            }
        }
        /* lane j: packet j's header and record */
        const unsigned length = 12u + (unsigned)(listed ? F : cn) * FB;
        for (int j = lane; j < np; j += 64) {
            if (first + j >= a.max_packets) continue;
            const unsigned seq = (st.seq + (unsigned)j) & 0xFFFFu, ts = ts_start + (uint32_t)(j * F);
            const unsigned marker = (listed && j == 0 && !(st.flags & 1u)) ? 1u : 0u;
            unsigned* const slot = reinterpret_cast<unsigned*>(a.packets + (long)(first + j) * a.slot_bytes);
            __builtin_nontemporal_store(0x80u | (((marker << 7) | (src.payload_type & 0x7Fu)) << 8) | ((seq >> 8) << 16) | ((seq & 0xFFu) << 24), slot);
            __builtin_nontemporal_store(__builtin_bswap32(ts), slot + 1);
            __builtin_nontemporal_store(__builtin_bswap32(src.ssrc), slot + 2);
            rtp_v4u rec;
            rec.x = (unsigned)c;
            rec.y = ts;
            rec.z = seq | (length << 16);
            rec.w = marker | (listed ? 0u : 2u); /* flags; reserved = 0 */
            __builtin_nontemporal_store(rec, reinterpret_cast<rtp_v4u*>(a.records + (first + j)));
        }
        RTP_CARRY_READ(); /* every lane has read the state and what it needs of the old carry */
        /* what is left of the row is the new carry: np >= 1 packets took at least F > cn frames, so it lies in the row */
        const int rem = listed ? rtp_clamp(cn + B - np * F, 0, a.carry_cap) : 0, rd = rem * FB / 4;
        for (int d = lane; d < rd; d += 64) carry[d] = __builtin_nontemporal_load(rowp + (Bd - rd) + d);
        if (lane == 0) {
            airband_hip_rtp_state n = st;
            n.packets = st.packets + (uint32_t)np;
            n.octets = st.octets + (uint32_t)(nd * 4);
            n.seq = (uint16_t)(st.seq + (unsigned)np);
            n.carry = (uint16_t)rem;
            n.flags = listed ? 1u : 0u;
            a.state[c] = n;
        }
    }
}

__global__ __launch_bounds__(64) void rtp_write_kernel(RtpArgs a) {
    /* uniform: one of four straight-line bodies, the frame size a compile-time constant in each */
    if (a.width_shift) {
        if (a.sample_bytes == 2)
            rtp_write<2, 2>(a);
        else
            rtp_write<1, 2>(a);
    } else if (a.sample_bytes == 2) {
        rtp_write<2, 1>(a);
    } else {
        rtp_write<1, 1>(a);
    }
}

void launch_rtp_step(const RtpArgs& a, int grid, hipStream_t stream) {
    const int nb = (a.n_ch + GATE_BLOCK - 1) / GATE_BLOCK; /* gate_blocks(): the gate's counts are per workgroup of this size */
    hipLaunchKernelGGL(rtp_count_kernel, dim3(nb), dim3(GATE_BLOCK), 0, stream, a);
    hipLaunchKernelGGL(rtp_scan_kernel, dim3(nb), dim3(GATE_BLOCK), 0, stream, a);
    int gx = grid > 0 ? grid : (a.n_ch < RTP_MAX_GRID ? a.n_ch : RTP_MAX_GRID);
    hipLaunchKernelGGL(rtp_write_kernel, dim3(gx < 1 ? 1 : gx), dim3(64), 0, stream, a);
}

}  // namespace airband
