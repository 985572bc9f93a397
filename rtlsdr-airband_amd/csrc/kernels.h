/* csrc/kernels.h -- launch interfaces of the HIP kernels (host side: airband_hip.cpp and driver_*.cpp, see driver.h). */
#ifndef AIRBAND_CSRC_KERNELS_H
#define AIRBAND_CSRC_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/airband_hip.h"
#include "common.h"
#include "dft_wide_map.h"

namespace airband {

/* Device buffers are blocked time-major rings (see ab_ring_base in common.h): logical row r of the current batch
 * lives at physical row (row0 + r) mod ring_rows, ring_rows = WAVE_BATCH + AGC_EXTRA.  Logical rows [0, AGC_EXTRA) are the carry from
 * the previous batch (what the reference keeps with its memmove / tail copy, src/rtl_airband.cpp:621-624 and
 * src/output.cpp:920), rows [AGC_EXTRA, AGC_EXTRA + WAVE_BATCH) are this batch's new hops.  Advancing row0 by
 * WAVE_BATCH per batch replaces both copies. */

struct ChannelizerArgs {
    const uint8_t* iq;      /* device: dongle d's span starts at iq + d * iq_stride */
    long iq_stride;         /* bytes */
    const DevConst* dev;
    const ChanState* cs;    /* for the (AFC-movable) bin of every slot */
    const ChanConst* cc;
    const int* ext_to_slot; /* channel (device-major external index) -> demod slot */
    const float* window;    /* fft_size */
    const float* window_dec;/* fft_size >= 1024: [fft_size / 512][512] the window at samples n2 + (fft_size / 512) n1, row n2 (decimated wavefront FFT); else unused */
    const float2* twiddle;  /* fft_size: exp(-2 pi i k / fft_size) */
    float* mag;             /* |bin| ring, blocked by 64 slots and transposed in tiles of AB_TILE_ROWS rows (common.h: ab_tile_base / ab_tile_off) */
    float2* iq_bins;        /* raw bin I/Q ring, same layout */
    float* last_spectrum;   /* [n_dev][2*fft_size] full FFT of the batch's last hop (AFC), or null */
    int n_dev, fft_log;
    int hop_samples, bytes_per_sample, sfmt;
    float scale;
    int row0, ring_rows;
    int first_row;          /* first logical row to produce (0 on the first batch, AGC_EXTRA later) */
    int n_hops;             /* hops to produce */
    int max_ch;
    int spectrum_only;      /* 1: no ring output, only last_spectrum of dongles with an AFC channel (handles whose batches run on the matrix-core channelizer) */
};

/* matrix-core channelizer (channelizer_dft.hip) */
struct DftArgs {
    const uint8_t* iq;
    long iq_stride;
    const DevConst* dev;
    const ChanConst* cc;
    const int* ext_to_slot;
    const int* item_dev;    /* [n_items] work items: (dongle, group of 8 channels, coefficient-table index) */
    const int* item_group;
    const int* item_bset;
    const int8_t* bfrag;    /* [n_bsets][window pieces][3 digits][k-steps][64 lanes][16 bytes] MFMA B fragments (k-steps = min(fft_size, 512) / 32) */
    const double* corr;     /* [n_bsets * window pieces][16] offset restoring (b - 127.5) from (b - 128), in table units */
    double unscale;         /* u8: 1 / (table scale * 127.5); CS16: 1 / table scale (the kernel multiplies by the dongle's 1 / fullscale) */
    float* mag;
    float2* iq_bins;
    int n_dev, n_items, splits, fft_size, sfmt;
    int piece0, np_total;            /* fft_size > 512: first window piece of this launch / number of pieces of the window (set by launch_channelizer_dft) */
    float4* partial;                 /* fft_size 8192 only: [n_items][tiles][64] partial sums between the two passes (dft_partial_tiles() tiles per item) */
    int edge_hi_zero;                /* most significant digit is zero in k-steps 0,1,14,15 for every coefficient table */
    int hop_bytes, lds_per_buf, sub, nbuf; /* sub = 16-hop MFMA tiles per staging step; nbuf staging buffers */
    int row0, ring_rows, first_row, n_hops;
    int extra_lds;          /* bytes of LDS the launch asks for beyond what it uses: run-ahead and AIRBAND_HIP_FLAG_PIPELINE handles hold the channelizer to five wavefronts per CU, so that
                             * every CU has register room for the stage-2 wavefronts of the batch before (airband_hip.cpp; profiles/r06_experiments.md I) */
};

/* CF32 dongles on the float32 matrix pipe (channelizer_f32.hip) */
struct F32Args {
    const uint8_t* iq;
    long iq_stride;
    const DevConst* dev;
    const ChanConst* cc;
    const int* ext_to_slot;
    const int* item_dev;    /* work items as for DftArgs: (dongle, group of 8 channels, coefficient-table index) */
    const int* item_group;
    const int* item_bset;
    const float* btab;      /* [n_bsets][f32_nw pieces][MFMAs per piece][64 lanes] window x twiddle, ordered as the kernel contracts (params.cpp, build_f32_tables) */
    float* mag;
    float2* iq_bins;
    int n_items, splits, fft_size;
    int hop_bytes, pad, lds_per_buf; /* bytes per hop (8 x hop_samples), padding per hop in the staged image, bytes per staging buffer */
    int row0, ring_rows, first_row, n_hops;
    int seg, n_seg;         /* fft_size 4096 / 8192 (wide hops: 2048 and up): window segment of this launch / segments per window (set by launch_channelizer_f32[_wide]) */
    float4* partial;        /* those sizes only: [n_items][f32_partial_tiles() tiles][64] partial sums between the segments' launches */
};

struct DemodArgs {
    const ChanConst* cc;
    ChanState* cs;
    float* mag;
    const float2* iq;
    float* out_wave;        /* [total_channels][wave_stride]: channel->waveout rows (tail + WAVE_BATCH), written directly */
    uint8_t* out_axc;       /* [total_channels] */
    const int* slot_to_ext;
    int wave_stride;
    int tail_copy;          /* 0 for the very first batch: nothing has been consumed yet */
    float2* iq_out;         /* [slot blocks][wave_batch][64] raw I/Q of open samples (channels with has_iq_outputs), emit_iq_kernel turns it channel-major */
    float* sqbuf;           /* [slot blocks][AB_SQ_BUF][64] the squelch's pre-filter delay line (ab_ring_base); only the generic kind still stores it -- the NFM + lowpass kind recomputes its entries (SqShadow) */
    const float* ct_coeff;  /* [n_ctcss][2 detectors][AB_MAX_TONES] */
    float* ct_q;            /* [n_ctcss][2 detectors][q1|q2][AB_MAX_TONES] */
    uint8_t* trace;         /* [slot blocks][wave_batch][64] per-sample squelch trace, or null */
    /* split (CTCSS-capable) kinds: front -> tone -> back hand-off */
    /* hand-off rows, channel-major (the tone kernel reads a channel's samples across its lanes):
     *   generic kind  [slots of the generic blocks][wave_batch] (pre-notch audio, flag word) pairs
     *   NFM + CTCSS   [slots of its blocks][ct_pk_pitch] one word per sample (demod.hip, HAND_WORD), rows of whole 128-byte lines */
    float2* ct_af;
    unsigned* ct_ap;
    int ct_pk_pitch;
    int ct_pk_first_block, ct_pk_n_blocks, ct_gen_first_block, ct_gen_n_blocks;
    unsigned long long* ct_mask;   /* [ct blocks][wave_batch / 50][64] tone-present bits, blocks counted from ct_first_block (both split kinds) */
    int ct_first_block, ct_n_blocks;
    const float* sin_lut;   /* 257 */
    const float* cos_lut;   /* 257 */
    int ct_stride;
    int n_slots, wave_batch, row0, ring_rows;
    /* REGROUPED handles (AIRBAND_HIP_FLAG_REGROUP, demod.hip "regrouping"): the lane-per-channel kernels run as workgroups of AB_REGROUP_WAVES wavefronts that
     * share AB_REGROUP_WAVES x 64 consecutive slots and deal them out among themselves by squelch state -- the channels that are not at rest in CLOSED to the first
     * wavefronts, the closed ones to the last, so that whole wavefronts of closed channels skip the open channels' instructions -- and walk the batch in step
     * (a workgroup barrier every eight samples), so that the ring lines neighbouring slots share are fetched from memory once.  Everything a lane touches is
     * addressed by its SLOT: which lane works on which slot does not change a result.  0: lane l of block b works on slot 64 b + l. */
    int regroup;
    /* regroup == 3 (round 6, third form): a per-batch permutation of every kind's slots, built by regroup_perm_kernel in front of the stage -- inside segments of sixteen
     * blocks the LINE GROUPS (slots that share a 128-byte ring line) with a channel that is not at rest come first, the groups at rest behind them -- read by ordinary
     * one-wavefront workgroups: lane l of block b works on slot perm[64 b + l].  Nothing is shared between wavefronts, nobody waits, no workgroup needs four slots at once. */
    int* perm;
    uint8_t* sq_key;        /* [n_slots] split kinds: the front kernel leaves 1 where the channel had audio or went CLOSED in this batch; the tone kernel skips the others, regrouped handles' back kernel deals its slots out by it */
};

struct EmitArgs { /* raw I/Q outputs only: audio goes straight to its channel row */
    const float2* iq_out;
    const int* slot_to_ext;
    float* out_iq;          /* [total_channels][2*wave_batch] or null */
    int n_slots, wave_batch;
};

struct MixArgs {
    const float* out_wave;  /* [total_channels][wave_stride] */
    int wave_stride;
    const uint8_t* out_axc;
    const int* in_chan;     /* [n_inputs] external channel index, grouped by mixer */
    const float* in_ml;     /* ampfactor * ampl */
    const float* in_mr;     /* ampfactor * ampr */
    const int* run_first;       /* [n_runs + 1] offsets into the input arrays: runs of <= AB_MIX_RUN inputs of one mixer */
    const int* run_mixer;       /* [n_runs] */
    const int* mixer_first_run; /* [n_mixers + 1] */
    const uint8_t* mixer_stereo;
    float* run_left;            /* [n_runs][wave_batch] stage-A sums */
    float* run_right;
    uint8_t* run_signal;        /* [n_runs] */
    float* left;            /* [n_mixers][wave_batch] */
    float* right;
    uint8_t* has_signal;    /* [n_mixers] */
    int n_mixers, n_runs, wave_batch;
};

struct SiggenArgs {
    uint8_t* iq;
    long stride;            /* bytes per dongle */
    const int16_t* sin_tab; /* 4096 */
    const long long* carriers; /* [n_carriers][12] */
    int n_carriers;
    int n_dev;
    int dev_offset;
    unsigned long long start_sample;
    long n_samples;
    unsigned long long seed;
    int noise_q8;
    /* fleets whose dongles do not share a channel plan (bench.py --distinct-plans): dongle `dev` belongs to plan p = dev mod n_plans, and its carrier c sits
     * ((p >> 2c) & 3) * plan_shift_step further up than the table says -- 4^8 = 65 536 distinct plans of eight carriers; n_plans <= 1: every dongle as the table says */
    int n_plans;
    unsigned plan_shift_step; /* u32 turns per sample */
};

void launch_channelizer_fft(const ChannelizerArgs& a, hipStream_t stream);
size_t fft_lds_bytes(int fft_log, int hop_samples, int bytes_per_sample); /* dynamic LDS per workgroup: prepare() refuses configurations above the CU's 160 KiB, the launch opts in above 64 KiB */
bool dft_supported(int fft_size, int hop_bytes, int sfmt, int max_ch);
int dft_lds_per_buf(int hop_bytes, int win_bytes, int np);
int dft_sub(int hop_bytes, int win_bytes, int np);
int dft_nbuf(int hop_bytes, int win_bytes, int np);
int dft_partial_tiles(int n_hops_max); /* 16-hop tiles a work item may touch in one launch (sizes DftArgs::partial) */
void launch_channelizer_dft(const DftArgs& a, hipStream_t stream);
/* wide hops (channelizer_dft_wide.hip, AIRBAND_HIP_FLAG_WIDE_HOPS): a tile is staged as 16 rows of one window each.  The geometry, shared by the kernel (as
 * constant expressions) and the host: win_all = bytes of a whole window, np = its pieces of 512 samples.  Row pitch = window + 16 (an odd number of 16-byte
 * bank columns, and room for the up-to-15 bytes in front of an unaligned row), a buffer = 16 rows in whole 1 KiB transfers, two buffers + the exchange area of
 * the window pieces' partial sums.  Windows whose two images do not fit are staged a k-segment at a time (dft_wide_map.h holds the geometry of both and the
 * address map; the three functions below are its one-segment case under the names the host code uses). */
constexpr int dft_wide_pitch(int win_all) { return wide_sub_pitch(win_all, 1, 1); }
constexpr int dft_wide_lds_per_buf(int win_all) { return wide_image_bytes(win_all, 1, 1); }
constexpr int dft_wide_lds_bytes(int win_all, int np) { return wide_lds_total(win_all / np, np, 1); }
/* dynamic LDS of the wide-hop kernel for this shape with whole windows staged (one segment), or -1 where the shape is not its business (hops inside
 * dft_supported()'s limits, odd hops, CF32) */
#define AB_DFT_WIDE_LDS_MAX airband::WIDE_LDS_MAX
int dft_wide_lds(int fft_size, int hop_bytes, int sfmt);
/* THE rule by which a flagged handle takes the wide-hop kernel: the smallest number of k-segments per window piece, 1 / 2 / 4, whose two images and exchange area
 * are at most AB_DFT_WIDE_LDS_MAX (dft_wide_map.h); *lds_bytes (may be null) = that plan's dynamic LDS.  0: no plan fits (fft_size 8192 is not tried: more than
 * eight pieces need the two-pass partial sums of channelizer_dft.hip; *spills (may be null) = true where a plan fits but its kernel variant is not built because it
 * spills registers: segments at u8 / s8 hops of an odd number of samples); -1: not a wide shape (as dft_wide_lds()). */
int dft_wide_plan(int fft_size, int hop_bytes, int sfmt, int* lds_bytes, bool* spills);
void launch_channelizer_dft_wide(const DftArgs& a, hipStream_t stream);
/* side: 3 extra streams, ev: 4 events (fork + 3 joins); both may be null -> everything on `stream`, one kind after the other */
void launch_demod(const DemodArgs& a, const int* kind_first_block, const int* kind_n_blocks, hipStream_t stream, hipStream_t* side, hipEvent_t* ev);
/* waves per workgroup = pieces the contraction index (2 fft_size values) is cut into: four up to fft_size 512 (64 / 32 resident B registers per wave), eight for 1024 and 2048
 * (64 / 128): a workgroup of eight waves is two per SIMD, which is what 128 B registers beside everything else allow anyway */
inline int f32_nw(int fft_size) { return fft_size <= 512 ? 4 : 8; }
/* fft_size 4096 / 8192: the window in segments of 2 048 samples, each contracted by the fft 2048 kernel with the segment's own table (one launch per segment) */
inline int f32_seg_size(int fft_size) { return fft_size < 2048 ? fft_size : 2048; }
inline int f32_n_seg(int fft_size) { return fft_size / f32_seg_size(fft_size); }
int f32_partial_tiles(int n_hops_max); /* 16-hop tiles a work item may touch in one launch (sizes F32Args::partial) */
/* layout of the staged image (channelizer_f32.hip): 1 = hops of an odd number of samples (no padding, fragments from two 8-byte reads), 3 = hops of an odd number of 16-byte units (no padding), 2 = 16 bytes of padding per 256 stream
 * bytes (hops that are multiples of 256 bytes; offsets become immediates), 0 = 16 bytes per hop where the hop is an even number of 16-byte units.  fft 512 with the small tiles
 * of WAVE_RATE 16000 stays on 0: layout 2's 6 % more LDS would cost it its third workgroup per CU (measured: 22.1 -> 24.1 ms; every other variant gains, fft 2048 27 %) */
/* THE small-tile rule (launch_channelizer_f32 picks MAX_LD = 6 or 12 by it): a tile's 16 hops of one window segment, plus the 16 bytes an image of odd hops may start in front of
 * the tile, within six 16-byte pieces per thread -- the register budget of three workgroups per CU (NW = 4) */
inline bool f32_small_tile(int fft_size, int hop_bytes) {
    return 15 * hop_bytes + 8 * f32_seg_size(fft_size) + ((hop_bytes & 8) ? 16 : 0) <= 6 * 64 * f32_nw(fft_size) * 16;
}
inline int f32_layout(int fft_size, int hop_bytes) {
    if (hop_bytes & 8) return 1;
    if ((hop_bytes / 16) & 1) return 3; /* an odd number of 16-byte units per hop (2.4 MS/s: 1 200 / 2 400 bytes): the rows fall in different bank groups as they are -- no padding, offsets are immediates */
    if (hop_bytes % 256) return 0;
    return (fft_size == 512 && f32_small_tile(fft_size, hop_bytes)) ? 0 : 2;
}
bool f32_supported(int fft_size, int hop_samples, int sfmt);
int f32_pad_bytes(int hop_samples);
int f32_lds_per_buf(int fft_size, int hop_samples);
void launch_channelizer_f32(const F32Args& a, hipStream_t stream);
/* CF32 wide hops (channelizer_f32_wide.hip, AIRBAND_HIP_FLAG_WIDE_HOPS): a tile is staged as 16 rows of one window segment each (f32_wide_map.h: geometry and address
 * map), one image in LDS and the next tile in registers.  THE rule by which a flagged CF32 handle takes it: the smallest power-of-two number of equal window segments
 * whose image and exchange area fit a CU's 163 840 bytes -- 1 up to fft 1024, then segments of 1 024 samples, one launch each through F32Args::partial.  Returns that
 * number (*segments the same, *lds_bytes the dynamic LDS of a launch; both may be null); 0: no plan; -1: not a wide shape (inside f32_supported()'s limits, or no fft
 * size of the float kernels). */
int f32_wide_plan(int fft_size, int hop_samples, int* segments, int* lds_bytes);
int f32_wide_seg_size(int fft_size); /* window samples per segment of that plan */
void launch_channelizer_f32_wide(const F32Args& a, hipStream_t stream);
void launch_emit_iq(const EmitArgs& a, hipStream_t stream);
void launch_axc(const ChanConst* cc, const ChanState* cs, const int* slot_to_ext, uint8_t* out_axc, int n_slots, hipStream_t stream);
void launch_mix(const MixArgs& a, hipStream_t stream);
/* dst += src for the mixer sums of two handles on one GPU (airband_hip_add_mixers): left, right [n_mixers][wave_batch], signal flags OR-ed */
void launch_mix_add(float* dl, float* dr, uint8_t* ds, const float* sl, const float* sr, const uint8_t* ss, int n_mixers, int wave_batch, hipStream_t stream);
void launch_stats(const ChanConst* cc, const ChanState* cs, const int* slot_to_ext, int n_slots, airband_hip_channel_stats* out, hipStream_t stream);
void launch_siggen(const SiggenArgs& a, hipStream_t stream);
void launch_afc(const ChanConst* cc, ChanState* cs, const float* spectrum, int fft_size, int n_slots, int* moved_epoch, int epoch, hipStream_t stream);
/* matrix-core channelizer + AFC: (re)builds, in place, the coefficient columns of every channel whose table is not built for the bin the channel
 * is tuned to now -- all columns of a private table at start-up (bset_bin = -1), the two columns of a channel AFC has just moved afterwards */
struct RetuneArgs {
    const ChanConst* cc;
    const ChanState* cs;
    const DevConst* dev;
    const int* ext_to_slot;
    const int* item_dev;
    const int* item_group;
    int* item_bset;         /* what the channelizer reads: item_home while every channel of the group sits on its base bin, item_private otherwise */
    const int* item_private;/* the group's own table (>= n_shared), or its shared one for groups without an AFC channel */
    const int* item_home;
    int* bset_bin;          /* [n_bsets][8] */
    int8_t* bfrag;
    double* corr;
    float* ftab;            /* CF32 handles (channelizer_f32.hip): the float tables instead of bfrag / corr (both null then); else null */
    const float* window;    /* fft_size */
    int n_items, fft_size, n_shared;
    const int* moved_epoch; /* the batch number afc_kernel stamped when it last moved a channel; the kernel works only if it equals `epoch` (start-up build: both 0) */
    int epoch;
};
void launch_retune(const RetuneArgs& a, hipStream_t stream);
/* shared coefficient tables [first, first + n) built on the device, every column from bset_bin[table][8] (the host builds the first few thousand of a fleet's distinct
 * channel plans, params.cpp; the rest here, at prepare() time) */
void launch_build_tables(int8_t* bfrag, double* corr, const float* window, const int* bset_bin, int first, int n, int fft_size, hipStream_t stream);
/* scatter channel-major host-provided bins into the time-major rings (airband_hip_process_bins) */
void launch_scatter_bins(const float* wavein, const float* iqin, const int* slot_to_ext, const ChanConst* cc, float* mag, float2* iq, int n_slots,
                         int wave_batch, int row0, int ring_rows, hipStream_t stream);
/* the batch's new stage-1 rows (and squelch trace) of channels [first, first + n), channel-major (airband_hip_read_bins / read_trace);
 * |bin| of NFM channels, which stage 1 does not store, is recomputed from the raw bin I/Q the way stage 2 does */
void launch_gather_channels(const float* mag, const float2* iq, const uint8_t* trace, const int* ext_to_slot, const ChanConst* cc, int first, int n, float* wavein,
                            float* iqin, uint8_t* trace_out, int wave_batch, int row0, int ring_rows, hipStream_t stream);

/* scan-mode devices (scan_bank.h): the per-frequency state banks and the batch's switch list */
struct ScanExchangeArgs {
    ChanConst* cc;          /* live, by slot */
    ChanState* cs;
    float* sqbuf;           /* the squelch delay lines, ab_ring_base(slot, AB_SQ_BUF) + 64 i */
    const ChanConst* bank_cc; /* [n_entries] read-only */
    ChanState* bank_cs;     /* [n_entries] */
    float* bank_sq;         /* [n_entries][AB_SQ_BUF] */
    const uint32_t* cs_mask;/* [AB_CS_DWORDS] */
    const uint32_t* cc_mask;/* [AB_CC_DWORDS] */
    const int* sw;          /* [n_switch][3] (slot, entry parked, entry brought in) */
    int n_switch, n_slots, n_entries;
};
void launch_scan_exchange(const ScanExchangeArgs& a, hipStream_t stream);
void launch_scan_compose(const ScanExchangeArgs& a, int slot, int e, ChanConst* out_cc, ChanState* out_cs, hipStream_t stream);
void launch_scan_mag(const int* slots, int n, float* mag, const float2* iq, int first_row, int n_rows, int row0, int ring_rows, hipStream_t stream);

/* signal-gated collect (gate.hip): the batch's active channels, ascending, and their rows packed */
#define AB_GATE_OFF 0x80u /* in a device-side gate byte: the channel's dongle is switched off (airband_hip_device_enable) */
struct GateArgs {
    const uint8_t* gate;      /* [n_ch] AIRBAND_GATE_*, | AB_GATE_OFF */
    const uint8_t* axc;       /* [n_ch] the batch's axcindicate */
    uint8_t* prev;            /* [n_ch] the channel had signal in the batch before */
    unsigned long long* mask; /* [ceil(n_ch / 64)] the verdicts, one bit per channel */
    int* block_count;         /* [gate_blocks(n_ch)] */
    int* index;               /* [max_rows] */
    int* count;               /* [1] channels the rule selected (may exceed max_rows) */
    int n_ch, max_rows;
    const float* out_wave;    /* row starts (AB_OUT_PAD is skipped by the kernel) */
    const float* out_iq;      /* [n_ch][2 * wave_batch], or null */
    float* rows;              /* [max_rows][wave_batch] */
    float* iq_rows;           /* [max_rows][2 * wave_batch], or null */
    int wave_stride, wave_batch;
};
int gate_blocks(int n_ch);
void launch_gate(const GateArgs& a, hipStream_t stream);

/* encoded audio collect (audio_pack.hip): rows as int16 or G.711 bytes and one record per row; one wavefront per row, workgroups stride over the rows */
struct AudioPackArgs {
    const int* index;         /* [max_rows] row r is channel index[r] (the gate's list); null: row r is source row r (airband_hip_encode_audio) */
    const int* count;         /* [1] on the device: the gate's count (may exceed max_rows); null: n_rows */
    int n_rows;
    int max_rows, n_ch;       /* the clamps: rows written, source rows there are */
    const float* src;         /* source row c starts at src + c * src_stride + src_pad, 16-byte aligned */
    long src_stride;
    int src_pad;
    void* audio;              /* [max_rows][wave_batch] int16 (S16) or bytes (G.711) */
    airband_hip_audio_row* info; /* [max_rows] */
    int wave_batch;           /* a multiple of four */
    int encoding;             /* AIRBAND_AUDIO_S16 / _ULAW / _ALAW */
};
void launch_audio_pack(const AudioPackArgs& a, int grid, hipStream_t stream); /* grid: workgroups, 0 = min(max_rows, one per wavefront slot of the GPU) */

/* output decimation by 2 (audio_decimate.hip), in launch_audio_pack's place on a decimating handle: rows of wave_batch / 2 samples as int16 or G.711 bytes and
 * one record per row, through the half-band FIR of audio_decimate.h with 46 carried values per channel; the same shape of launch */
struct AudioDecimateArgs {
    const int* index;         /* [max_rows] row r is channel index[r] (the gate's list); null: row r is source row r (airband_hip_decimate_audio) */
    const int* count;         /* [1] on the device: the gate's count (may exceed max_rows); null: n_rows */
    int n_rows;
    int max_rows, n_ch;       /* the clamps: rows written, source rows (and histories) there are */
    const float* src;         /* source row c starts at src + c * src_stride + src_pad, 16-byte aligned */
    long src_stride;
    int src_pad;
    void* audio;              /* [max_rows][wave_batch / 2] int16 (S16) or bytes (G.711) */
    airband_hip_audio_row* info; /* [max_rows] */
    int16_t* hist;            /* [n_ch][46] the q values a channel carries, read and written back; null: zeros in, nothing out */
    uint32_t* stamp;          /* [n_ch] the last step that listed the channel: its history counts only if that is k - 1; null: it always counts */
    uint32_t k;               /* the step's number, 1, 2, ... (a zeroed stamp is "listed in step 0", with the zeroed history every channel starts from) */
    int wave_batch;           /* a multiple of eight */
    int encoding;             /* AIRBAND_AUDIO_S16 / _ULAW / _ALAW */
};
size_t audio_decimate_lds_bytes(int wave_batch); /* the launch's dynamic LDS */
void launch_audio_decimate(const AudioDecimateArgs& a, int grid, hipStream_t stream); /* grid: as launch_audio_pack's */

/* gated mixer collect (mixer_gate.hip): the batch's active mixers, ascending (gate_passes.h), and their rows packed as float32, int16 or G.711 frames */
struct MixerGateArgs {
    const uint8_t* gate;       /* [n_mixers] AIRBAND_GATE_* */
    const uint8_t* has_signal; /* [n_mixers] the sums' signal flags at the step */
    uint8_t* prev;             /* [n_mixers] the mixer had signal at the step before */
    unsigned long long* mask;  /* [ceil(n_mixers / 64)] */
    int* block_count;          /* [gate_blocks(n_mixers)] */
    int* index;                /* [max_rows] */
    int* count;                /* [1] mixers the rule selected (may exceed max_rows) */
    int n_mixers, max_rows;
};
struct MixerPackArgs {
    const int* index;          /* [max_rows] row r is mixer index[r]; null: row r is source row r (airband_hip_encode_mixer_audio) */
    const int* count;          /* [1] on the device (may exceed max_rows); null: n_rows */
    int n_rows;
    int max_rows, n_mixers;    /* the clamps: rows written, source rows there are */
    const float* left;         /* [n_mixers][wave_batch], rows 16-byte aligned */
    const float* right;        /* likewise; read only when width == 2 */
    const uint8_t* stereo;     /* [n_mixers] the mixers' stereo flags -> the record's `reserved`; null: `reserved_all` */
    unsigned reserved_all;
    void* out;                 /* [max_rows][width * wave_batch] float32, int16 or bytes */
    airband_hip_audio_row* info; /* [max_rows]; not written for AIRBAND_AUDIO_F32 */
    int wave_batch;            /* a multiple of four */
    int encoding;              /* AIRBAND_AUDIO_* */
    int width;                 /* 1: frames of left; 2: frames of (left, right) */
};
void launch_mixer_gate_list(const MixerGateArgs& a, hipStream_t stream);
void launch_mixer_pack(const MixerPackArgs& a, int grid, hipStream_t stream); /* grid: workgroups, 0 = min(max_rows, one per wavefront slot of the GPU) */

/* transmission spool (tx_spool.hip): the encoded rows of every open transmission kept in a row pool, the closing rule applied once per batch, finished
 * transmissions listed in (step, channel) order and exported as one contiguous run of rows.  Written against "a mask, counts, rows, records": the channel spool
 * fills SpoolArgs from the output gate and the encoder, the mixer spool from the mixer gate and the mixer pack (n_ch = mixer_count, row_bytes = W * wave_batch * bytes) */
struct SpoolChan {
    uint32_t open_batch, last_batch, n_rows, n_lost;
    uint32_t n_clipped;
    uint16_t peak, first, end, open; /* open: the channel has an open transmission; nothing else means anything without it */
    int32_t head, tail;              /* its chain of pool rows (SpoolArgs::next); -1 while it has none */
    uint32_t flags;                  /* OR of the stored rows' airband_hip_audio_row.reserved: the record's reserved[1] */
    uint32_t pad[2];
}; /* 48 bytes */
static_assert(sizeof(SpoolChan) == 48, "SpoolChan is 48 bytes");
struct SpoolCtl {
    int32_t exp[3];                  /* the last collect's: transmissions exported, their rows, transmissions still waiting */
    int32_t free_top;                /* rows on the free stack */
    int32_t fin_head, fin_count;     /* the finished list: a ring of max_records records */
    int32_t room, fin_tail;          /* of the running step (written by the scan pass): records the list can take, where they go */
    int32_t n_stored_step;           /* rows stored by the running step: summed by the append pass, applied by the copy pass */
    int32_t pad;
    unsigned long long open_now, finished_total, dropped, rows_stored, rows_lost;
};
struct SpoolArgs {
    const uint8_t* spool;            /* [n_ch] the channel is spooled */
    SpoolChan* chan;                 /* [n_ch] */
    SpoolCtl* ctl;                   /* [1] */
    unsigned long long* close_mask;  /* [ceil(n_ch / 64)] phase A's verdicts */
    unsigned long long* app_mask;    /* [ceil(n_ch / 64)] phase B's channels: spooled and selected */
    int* close_count;                /* [gate_blocks(n_ch)] */
    int* app_count;                  /* [gate_blocks(n_ch)] */
    const unsigned long long* gate_mask; /* the gate's verdicts and counts of this batch (GateArgs::mask, ::block_count) */
    const int* gate_count;
    int* free_stack;                 /* [pool_rows] */
    int* next;                       /* [pool_rows] the row behind this one in its chain, -1 */
    uint8_t* pool;                   /* [pool_rows][row_bytes] */
    int* copy_list;                  /* [max_rows][2] (encoded row, pool row) of the step's stored rows, by rank */
    const uint8_t* enc_audio;        /* the encoder's rows and records of this batch (AudioPackArgs::audio, ::info) */
    const airband_hip_audio_row* enc_info;
    airband_hip_transmission* fin;   /* [max_records] the ring; reserved[0] holds the chain's head while a record waits */
    airband_hip_transmission* exp_records; /* [max_records] */
    int* exp_head;                   /* [max_records] the exported transmissions' chains */
    int* exp_src;                    /* [export_rows] the pool row of every exported row */
    uint8_t* exp_audio;              /* [export_rows][row_bytes] */
    int n_ch, max_rows;              /* the gate's */
    int pool_rows, export_rows, max_records;
    int row_bytes;                   /* a multiple of four */
    int wave_batch;
    uint32_t min_batches, idle_batches, max_batches;
    uint32_t k;                      /* the step's number; flush: the steps run so far */
};
void launch_spool_step(const SpoolArgs& a, hipStream_t stream);    /* four launches: scan, close, append, copy */
void launch_spool_flush(const SpoolArgs& a, hipStream_t stream);   /* two: scan, close */
void launch_spool_collect(const SpoolArgs& a, hipStream_t stream); /* three: export, walk, gather */

/* RTP packet stream (rtp_stream.hip): the encoded rows a gate lists cut into RTP packets of frame_samples, the remainder carried per channel, one record per
 * packet, ranked (channel, time) by prefix sums.  Written against "a mask, counts, encoded rows": the driver fills them from the output gate and the encoder, or
 * from the mixer gate and the mixer pack ("channel" is then the mixer, a row wave_batch FRAMES of 1 << width_shift samples) */
struct RtpPlan {
    int32_t np, row;                 /* packets the step gives the channel; its row in the encoder's buffer, -1: not listed */
};
struct RtpWork {
    int32_t channel, first, row, pad; /* a channel with packets: its first slot, its row (-1: the flush packet) */
};
struct RtpBlock {
    int32_t packets, work, lost, octets; /* sums over one workgroup's channels */
};
struct RtpCtl {
    int32_t n_packets;               /* the step's packets (may exceed max_packets) */
    int32_t n_work;                  /* channels with packets in the step */
    int32_t pad[2];
    unsigned long long packets, dropped, octets, lost_rows;
};
struct RtpArgs {
    const airband_hip_rtp_source* sources; /* [n_ch] */
    airband_hip_rtp_state* state;    /* [n_ch] */
    uint8_t* carry;                  /* [n_ch][carry_stride] encoded samples */
    RtpCtl* ctl;                     /* [1] */
    RtpPlan* plan;                   /* [n_ch] */
    RtpBlock* blocks;                /* [gate_blocks(n_ch)] */
    RtpWork* work;                   /* [n_ch] */
    const unsigned long long* gate_mask; /* the gate's verdicts and counts of this step (GateArgs::mask, ::block_count; MixerGateArgs'), BOTH NULL: nobody is listed (the flush) */
    const int* gate_count;
    const uint8_t* enc_audio;        /* the encoder's rows of this step (AudioPackArgs::audio, MixerPackArgs::out) */
    airband_hip_rtp_packet* records; /* [max_packets] */
    uint8_t* packets;                /* [max_packets][slot_bytes] */
    int n_ch, max_rows;              /* the gate's */
    int wave_batch, frame_samples;   /* FRAMES of a row and of a packet: multiples of four */
    int sample_bytes;                /* 1 or 2 */
    int carry_cap;                   /* the longest carry in frames: frame_samples - gcd(wave_batch, frame_samples) */
    int carry_stride;                /* bytes of a channel's carry buffer: carry_cap * (sample_bytes << width_shift) */
    int slot_bytes, max_packets;
    uint32_t k;                      /* the step's number; flush: the steps run so far */
    int width_shift;                 /* a frame is 1 << width_shift samples: 0 (channels, mono mixer gates) or 1 (AIRBAND_MIXER_GATE_STEREO: L, R interleaved) */
};
void launch_rtp_step(const RtpArgs& a, int grid, hipStream_t stream); /* three launches: count, scan, write; grid: workgroups of the write pass, 0 = min(n_ch, one per wavefront slot of the GPU) */

/* band scope (band_scope.hip): mean and peak of |X[k]|^2 over n_windows windows of the batch's input span, one workgroup per selected dongle */
struct ScopeArgs {
    const uint8_t* iq;        /* device: dongle d's span starts at iq + d * iq_stride (the batch's stage-1 input) */
    long iq_stride;           /* bytes */
    const DevConst* dev;
    const int* dev_of_row;    /* [n_rows] the selected dongles, ascending */
    const float* window;      /* fft_size: the channelizer's window (params.cpp) */
    const float2* twiddle;    /* fft_size: exp(-2 pi i k / fft_size) */
    float* mean;              /* [n_rows][fft_size], or null */
    float* peak;              /* [n_rows][fft_size], or null */
    const float* prev_mean;   /* handles with two sets of rows: the set of the batch before, from which a switched-off dongle's rows are carried over; else null */
    const float* prev_peak;
    int n_rows, fft_log;
    int hop_samples, bytes_per_sample, sfmt;
    int first_hop;            /* hops of the span in front of the batch's new ones (the first batch's AGC_EXTRA lead-in, else 0) */
    int span_hops;            /* hops the span holds: first_hop + wave_batch */
    int wave_batch, n_windows;/* window j of n_windows = new hop (j * wave_batch) / n_windows */
    int region_bytes;         /* LDS per wavefront (set by launch_band_scope) */
};
long scope_region_bytes(int fft_log, int bytes_per_sample);
int scope_waves(int fft_log, int bytes_per_sample); /* wavefronts per workgroup: four where four regions fit a CU's 160 KiB, else two, else one */
void launch_band_scope(const ScopeArgs& a, hipStream_t stream);

/* band survey (band_survey.hip): noise floor, strongest bin and the unconfigured carriers of every row of one scope trace, one workgroup per row; launched
 * directly behind launch_band_scope() on the same stream */
struct SurveyArgs {
    const float* rows;        /* [n_rows][fft_size]: the scope trace's rows of this batch (ScopeArgs::mean or ::peak) */
    const int* bin_first;     /* [n_rows + 1] a row's channel bins are bins[bin_first[row] .. bin_first[row + 1]): at most AB_MAX_CH_PER_DEV */
    const int* bins;          /* prepare-time bins (ChanConst::base_bin) of the row's dongle */
    airband_hip_band_summary* summary; /* [n_rows] */
    airband_hip_band_peak* peaks;      /* [n_rows][max_peaks] */
    int n_rows, fft_log;
    int max_peaks;            /* 1 .. 64 */
    int rank;                 /* min(fft_size - 1, fft_size * floor_permille / 1000) */
    int guard_bins;           /* -1: no bin is covered */
    float ratio;              /* threshold = floor * ratio */
};
size_t survey_lds_bytes(int fft_log); /* dynamic LDS per workgroup: the row and 1.5 KiB */
void launch_band_survey(const SurveyArgs& a, hipStream_t stream);

/* band watch (band_watch.hip): the carrier tracks of every scope row advanced by the row's survey, one wavefront per row, and the rows' events packed into one
 * fleet-wide list in row order; launched directly behind launch_band_survey() on the same stream */
struct WatchArgs {
    const DevConst* dev;
    const int* dev_of_row;                      /* [n_rows] the selected dongles, ascending */
    const airband_hip_band_summary* summary;    /* [n_rows] the survey of this batch: n_peaks */
    const airband_hip_band_peak* peaks;         /* [n_rows][max_peaks] */
    const airband_hip_band_track* tracks_in;    /* [n_rows][max_tracks] the tables the batch starts from: the set of the batch before (== tracks_out on a handle with one set) */
    const airband_hip_band_watch_row* rows_in;  /* [n_rows] */
    airband_hip_band_track* tracks_out;
    airband_hip_band_watch_row* rows_out;
    airband_hip_band_event* stage;              /* [n_rows][max_peaks + max_tracks] a row's events of this batch, rows_out[row].n_events of them */
    airband_hip_band_event* events;             /* [max_events] */
    int* n_events;                              /* [1] */
    int n_rows, fft_log;
    int max_peaks;                              /* 1 .. 64: the survey's */
    int max_tracks;                             /* 1 .. 64 */
    int match_bins, confirm_hits, release_misses;
    int max_events;
    uint32_t batch;                             /* the watch batch number k */
};
void launch_band_watch(const WatchArgs& a, hipStream_t stream);

/* band follow (band_follow.hip): every scope row's followers decided against the row's track table as the watch left it, one wavefront per row; a follower that
 * changes has its ChanState::bin written and the re-tune epoch stamped there and then, and the rows' changes are packed into one fleet-wide list in row order.
 * Launched on the batch's stage-2 stream behind the demod kernels (which own ChanState) and behind the batch's watch. */
struct FollowArgs {
    const DevConst* dev;
    const int* dev_of_row;                      /* [n_rows] the selected dongles, ascending */
    const airband_hip_band_track* tracks;       /* [n_rows][max_tracks] the watch's tables of this batch */
    const int* fol_range;                       /* [n_rows][2] the row's followers: first (index in prepare order) and count (<= 64) */
    const int* fol_slot;                        /* [n_follow] the follower's demod slot */
    const int* fol_home;                        /* [n_follow] its home bin (ChanConst::base_bin) */
    airband_hip_band_follower* followers;       /* [n_follow] prepare order, advanced in place */
    airband_hip_band_follow_row* rows;          /* [n_rows] */
    airband_hip_band_follow_change* stage;      /* [n_rows][cap] a row's changes of this batch, rows[row].n_changes of them */
    airband_hip_band_follow_change* changes;    /* [max_changes] */
    int* n_changes;                             /* [1] */
    ChanState* cs;                              /* by slot: a changed follower's bin is written here */
    int* moved_epoch;                           /* the re-tune kernel's stamp (RetuneArgs::moved_epoch), or null where no coefficient table follows the bins */
    int epoch;
    int n_rows, n_follow, n_slots, fft_log;
    int max_tracks;                             /* 1 .. 64: the watch's */
    int cap;                                    /* most followers of a row + max_tracks */
    int max_changes;
    uint32_t batch;                             /* the watch batch number k of this batch */
};
void launch_band_follow(const FollowArgs& a, hipStream_t stream);

/* scan control (scan_control.hip): every scan list's hop decision of the batch, one thread per list, and the lists' records packed into one fleet-wide list in
 * dongle order.  Launched on the batch's stage-2 stream behind everything that writes the batch's axcindicate; the switch list it leaves is what the exchange
 * kernel in front of the next batch's demod kernels reads (ScanExchangeArgs::sw). */
struct ScanCtlList {
    int32_t dev, ext, slot;  /* the list's dongle, its channel (device-major) and that channel's demod slot */
    int32_t first_entry, n;  /* its entries in the banks: [first_entry, first_entry + n) */
    int32_t pad[3];
}; /* 32 bytes */
struct ScanControlArgs {
    const DevConst* dev;
    const uint8_t* axc;              /* [n_ch] the batch's axcindicate */
    const ScanCtlList* lists;        /* [n_lists] ascending dongle order */
    airband_hip_scan_state* state;   /* [n_lists] advanced in place */
    airband_hip_scan_event* stage;   /* [n_lists] a list's record of this batch, stage_n[list] of them (0 or 1) */
    int* stage_n;                    /* [n_lists] */
    int* sw;                         /* [n_lists][3] (slot or -1, entry parked, entry brought in) */
    airband_hip_scan_event* events;  /* [max_records] */
    int* n_events;                   /* [1] */
    int n_lists, n_dev, n_ch;
    int idle_batches, dwell_batches; /* >= 1 */
    int max_records;
    uint32_t batch;                  /* the control's batch number k */
};
void launch_scan_control(const ScanControlArgs& a, hipStream_t stream);
/* AB_F_VALID of one slot's live ChanConst::flags set or cleared in stream order, the other bits left as the exchange put them (airband_hip_device_enable on a
 * handle whose host copy of a scan slot's flags does not follow the GPU's hops) */
void launch_scan_set_valid(ChanConst* cc, int slot, int n_slots, int on, hipStream_t stream);

}  // namespace airband
#endif
