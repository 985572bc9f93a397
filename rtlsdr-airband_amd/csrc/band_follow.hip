/* csrc/band_follow.hip -- the band follow: spare channels (followers) tuned by the GPU onto the carriers the band watch has confirmed
 * (airband_hip_prepare_follow, airband_hip_set_band_follow).  Per scope row the decision which follower goes to which track, when it moves with the track and when
 * it goes home; the change is applied to the follower's ChanState::bin there and then, and one fleet-wide packed list holds the batch's changes.
 *
 * For every row, with T = max_tracks slots as the watch left them after this batch, the row's F <= 64 followers in ascending channel order, each
 * {track = slot or -1, bin, since_batch}, and the watch batch number k (include/airband_hip.h has the normative text) --
 *     A. every follower with a track s: tracks[s] not CONFIRMED: home (bin = home bin, track = -1, since_batch = k, a HOME change); else tracks[s].bin != bin:
 *        bin = tracks[s].bin, a MOVE change;
 *     B. every slot s ascending that is CONFIRMED and followed by no follower after A: the lowest follower that was idle at the start of the batch and is not
 *        taken yet takes it (track = s, bin = tracks[s].bin, since_batch = k, a TUNE change); none: the slot stays unserved.
 * capi.band_follow_reference() (rtlsdr-airband_amd/capi.py) is this definition in plain Python; tests/test_host_band_follow.py runs this file on the CPU against it.
 *
 * Mapping (wave64, CDNA4): the watch's.  band_follow_kernel: ONE WAVEFRONT per row, four rows per workgroup, no workgroup barrier and no LDS.
 *   * lane s holds slot s (state and bin: two registers), lane f holds follower f (16 bytes), its home bin and its demod slot;
 *   * step A: a follower reads its track's state and bin from lane `track` (two shuffles); the changes go to the row's staging slice at the lane's rank in the
 *     ballot of the changing followers = follower order;
 *   * "followed by no follower": every slot lane compares its number with each follower's track, broadcast by readlane in a wave-uniform loop of F rounds (F is 1
 *     or 2 on a fleet of eight-channel dongles), and the unserved slots are a ballot;
 *   * step B: a wave-uniform loop over min(unserved, idle) rounds: the lowest set bit of the ballot of the unserved slots and the lowest set bit of the ballot of
 *     the idle followers are paired and cleared; the follower's lane takes the slot's bin (readlane) and writes the change at a running wave-uniform index;
 *   * a changed follower's lane writes ChanState::bin of its slot and the re-tune stamp (every writer stores the same number, as afc_kernel's do): the launch
 *     sits on the batch's stage-2 stream behind the demod kernels, which own ChanState, and in front of the re-tune kernel;
 *   * the row record is written by lane 0.
 * A switched-off dongle (DevConst::disabled) is frozen: followers, bins and record stay, n_changes = 0.
 * band_follow_pack_kernel: the rows' changes into the fleet's list in row order (band_pack.h, the watch's scheme).
 * Integer arithmetic throughout, no atomics, every store by the lane that holds the value: equal input, equal bytes.
 * Every index is clamped to its buffer before use: a row's follower range to [0, n_follow) and 64, a follower's track to [0, T), its demod slot to [0, n_slots),
 * a track's bin to [0, fft_size) (it becomes the channelizer's bin), a staging index to cap = most followers of a row + T (at most F changes in step A and at
 * most T in step B by construction, checked again where it is used).
 */
#include <hip/hip_runtime.h>

#include "band_pack.h"
#include "common.h"
#include "kernels.h"

namespace airband {

namespace {

constexpr int FOLLOW_ROWS = 4, FOLLOW_THREADS = 64 * FOLLOW_ROWS;

typedef unsigned long long u64;

__device__ __forceinline__ airband_hip_band_follow_change make_change(int dev, int channel, int bin, int kind, int track) {
    airband_hip_band_follow_change c;
    c.dev = dev;
    c.channel = channel;
    c.bin = bin;
    c.kind = (uint8_t)kind;
    c.track = (uint8_t)track;
    c.reserved = 0;
    return c;
}

}  // namespace

__global__ __launch_bounds__(FOLLOW_THREADS) void band_follow_kernel(FollowArgs a) {
    const int lane = (int)threadIdx.x & 63;
    const int row = (int)blockIdx.x * FOLLOW_ROWS + ((int)threadIdx.x >> 6);
    if (row >= a.n_rows) return; /* wavefront-uniform */
    const int T = a.max_tracks, N = 1 << a.fft_log, cap = a.cap;
    const int d = a.dev_of_row[row];
    if (a.dev[d].disabled) { /* wavefront-uniform: frozen */
        if (lane == 0) a.rows[row].n_changes = 0;
        return;
    }
    int first = a.fol_range[2 * row], F = a.fol_range[2 * row + 1];
    first = first < 0 ? 0 : first;
    first = first > a.n_follow ? a.n_follow : first;
    F = F < 0 ? 0 : F;
    F = F > 64 ? 64 : F;
    F = F > a.n_follow - first ? a.n_follow - first : F;
    F = __builtin_amdgcn_readfirstlane(F);
    airband_hip_band_follow_change* const stage = a.stage + (long)row * cap;

    /* lane s: slot s */
    int tconf = 0, tbin = 0;
    if (lane < T) {
        const airband_hip_band_track t = a.tracks[(long)row * T + lane];
        tconf = t.state == AIRBAND_WATCH_CONFIRMED ? 1 : 0;
        tbin = t.bin < 0 ? 0 : t.bin;
        tbin = tbin > N - 1 ? N - 1 : tbin;
    }
    /* lane f: follower f */
    const bool mine = lane < F;
    airband_hip_band_follower fo;
    fo.channel = 0;
    fo.bin = 0;
    fo.since_batch = 0;
    fo.track = -1;
    fo.reserved = 0;
    int home = 0, slot = -1;
    if (mine) {
        fo = a.followers[first + lane];
        home = a.fol_home[first + lane];
        slot = a.fol_slot[first + lane];
    }
    int ftrack = mine && fo.track >= 0 && fo.track < T ? (int)fo.track : -1;
    const bool idle0 = mine && ftrack < 0; /* idle at the start of the batch */

    /* ---- A. the followers that have a track ---- */
    const int src = ftrack < 0 ? 0 : ftrack;
    const int sconf = __shfl(tconf, src), sbin = __shfl(tbin, src);
    int kind = 0;
    const int had = ftrack;
    if (ftrack >= 0) {
        if (!sconf) {
            fo.bin = home;
            fo.track = -1;
            fo.since_batch = a.batch;
            ftrack = -1;
            kind = AIRBAND_FOLLOW_HOME;
        } else if (sbin != fo.bin) {
            fo.bin = sbin;
            kind = AIRBAND_FOLLOW_MOVE;
        }
    }
    const u64 am = __ballot(kind != 0);
    if (kind != 0) {
        const int at = __builtin_popcountll(am & ((1ull << lane) - 1ull));
        if (at < cap) stage[at] = make_change(d, fo.channel, fo.bin, kind, had);
    }
    int nc = __builtin_popcountll(am); /* wavefront-uniform */

    /* ---- B. the confirmed slots nobody follows, in slot order ---- */
    bool followed = false;
#pragma unroll 1
    for (int f = 0; f < F; f++) followed |= (int)__builtin_amdgcn_readlane(ftrack, f) == lane;
    u64 um = __ballot(lane < T && tconf && !followed), im = __ballot(idle0);
#pragma unroll 1
    while (um != 0 && im != 0) {
        const int s = __builtin_ctzll(um), f = __builtin_ctzll(im);
        um &= um - 1;
        im &= im - 1;
        const int b = (int)__builtin_amdgcn_readlane(tbin, s);
        if (lane == f) {
            fo.track = (int16_t)s;
            fo.bin = b;
            fo.since_batch = a.batch;
            ftrack = s;
            kind = AIRBAND_FOLLOW_TUNE;
            if (nc < cap) stage[nc] = make_change(d, fo.channel, b, AIRBAND_FOLLOW_TUNE, s);
        }
        nc++;
    }

    /* ---- the followers, their channels' bins and the row record ---- */
    const u64 fm = __ballot(mine && ftrack >= 0);
    if (mine) a.followers[first + lane] = fo;
    if (kind != 0) {
        if (a.cs && slot >= 0 && slot < a.n_slots) a.cs[slot].bin = fo.bin;
        if (a.moved_epoch) *a.moved_epoch = a.epoch; /* some channel moved in this batch: the re-tune kernel has work (every writer stores the same number) */
    }
    if (lane == 0) {
        airband_hip_band_follow_row rr;
        rr.n_following = __builtin_popcountll(fm);
        rr.n_unserved = __builtin_popcountll(um);
        rr.n_changes = nc < cap ? nc : cap;
        rr.reserved = 0;
        a.rows[row] = rr;
    }
}

__global__ __launch_bounds__(PACK_THREADS) void band_follow_pack_kernel(FollowArgs a) {
    pack_rows(&a.rows[0].n_changes, (int)(sizeof(airband_hip_band_follow_row) / sizeof(int)), reinterpret_cast<const uint4*>(a.stage), a.cap,
              reinterpret_cast<uint4*>(a.changes), a.max_changes, a.n_changes, a.n_rows);
}

void launch_band_follow(const FollowArgs& a, hipStream_t stream) {
    if (a.n_rows <= 0 || a.n_follow <= 0 || a.max_tracks < 1 || a.max_tracks > 64 || a.cap < a.max_tracks) return;
    hipLaunchKernelGGL(band_follow_kernel, dim3((unsigned)((a.n_rows + FOLLOW_ROWS - 1) / FOLLOW_ROWS)), dim3(FOLLOW_THREADS), 0, stream, a);
    hipLaunchKernelGGL(band_follow_pack_kernel, dim3(1), dim3(PACK_THREADS), 0, stream, a);
}

}  // namespace airband
