/* csrc/channelizer_f32_wide.hip -- stage 1 for CF32 dongles whose hops are beyond channelizer_f32.hip's contiguous staging (AIRBAND_HIP_FLAG_WIDE_HOPS): above
 * ~3 MS/s at WAVE_RATE 8000, ~6 MS/s at 16000, up to any hop -- 20 MS/s (2 500 samples, 20 000 bytes per hop) included, which no other kernel of this project takes.
 *
 * The contraction is channelizer_f32.hip's, unchanged: v_mfma_f32_16x16x4_f32, float32 products and sums, the contraction index split over the workgroup's waves
 * (wave p owns window samples [S p / NW, S (p + 1) / NW)), resident B fragments read from the SAME tables in the same order (params.cpp, build_f32_tables: the table
 * is linear in the contraction index, so it serves any cut into segments and pieces), two accumulators, the finishing wave that rotates with the workgroup, the
 * ring stores and the XCD-aware work-item order.  From mfma_front.h: work_item(), tile_range(), split_share(), f32_exchange_put(), f32_exchange_sum(), opt_in_big_lds().  A flagged handle inside f32_supported()'s limits never comes here.
 *
 * What differs is the staging.  The ordinary kernel stages the 16 hops of a tile as ONE contiguous piece of the stream, 15 hops + a window long: at these hops
 * that is mostly bytes between windows, and it is what overflows LDS.  Here a tile is staged as 16 ROWS, row r = the S window samples of hop r that this launch
 * contracts, and the bytes between windows are never fetched.  The image is 16 x (8 S + 16) bytes whatever the hop (f32_wide_map.h: the address map, shared with
 * the host harness tests/host_f32_wide_map.cpp).  The pitch is an odd number of 16-byte units by construction: no per-hop padding arithmetic, no layout variants;
 * every LDS offset of a lane is a base register plus an immediate.
 *
 * ONE image in LDS, the next tile in registers: all threads fetch tile t + 1 with coalesced 16-byte global loads (a row is consecutive lanes) before the MFMAs of
 * tile t, and park it behind them, between two barriers.  Two images would not fit at S = 1024 (2 x 128 KiB); one leaves fft 512 two workgroups per CU, whose
 * MFMAs cover each other's parking, and fft 256 three.
 *
 * Hops of an odd number of samples (AL8; 625 samples at 10 MS/s, WAVE_RATE 16000) are 8 mod 16 bytes long: rows start alternately 0 and 8 bytes behind an aligned
 * 16-byte piece.  A row is staged from that aligned piece (one piece more per row, fetched by the workgroup's first sixteen threads) and the A fragments are
 * assembled from two 8-byte LDS reads at the row's own offset, as the ordinary kernel's AL8 variant does.  The span itself may start 8 bytes off a 16-byte boundary
 * then (the alignment rule of airband_hip_process_device for hops that are no multiple of 16 bytes); nothing is read past the span's last byte -- the span's last
 * piece is fetched as 8 bytes where only its first half belongs to the span -- and at most 8 bytes in front of it, inside the aligned piece that holds its first.
 *
 * Windows longer than one staged segment (fft_size 2048 and up: segments of 1 024 samples) run one launch per segment through F32Args::partial, as fft 4096 / 8192
 * do on the ordinary kernel. */
#include <hip/hip_runtime.h>
#include <atomic>

#include "common.h"
#include "f32_wide_map.h"
#include "kernels.h"
#include "mfma_front.h"

namespace airband {

namespace {

typedef float v2f __attribute__((ext_vector_type(2)));
typedef unsigned v4u __attribute__((ext_vector_type(4))); /* (not HIP's uint4: an array of that class type ends up in scratch memory) */
typedef unsigned v2u __attribute__((ext_vector_type(2)));

static_assert(TILE_HOPS == F32W_TILE_HOPS, "f32_wide_map.h plans for the tiles of mfma_front.h");

/* S: window samples staged per launch (256, 512, 1024); NW = f32w_nw(S) waves; AL8: hops of an odd number of samples */
template <int S, int NW, bool AL8>
__global__ __launch_bounds__(64 * NW, S == 256 ? 3 : 2) void channelizer_f32_wide_kernel(F32Args a) {
    constexpr int THREADS = 64 * NW;
    constexpr int KW = 2 * S / 4 / NW;      /* MFMAs per wave and tile = resident B registers: 32 (S = 256), 64 (512, 1024) */
    constexpr int READS = KW / 4;           /* 16-byte fragment reads per wave and tile */
    constexpr int NPR = S / 2;              /* 16-byte pieces of a row (AL8: + 1) */
    constexpr int RPI = THREADS / NPR;      /* rows the workgroup fetches per step: 2 (S = 256), 1 */
    constexpr int ROW_STEPS = TILE_HOPS / RPI;
    constexpr int MAX_LD = ROW_STEPS + (AL8 ? 1 : 0);
    static_assert(THREADS % NPR == 0 && TILE_HOPS % RPI == 0 && RPI >= 1, "a fetch step is whole rows");
    static_assert(NW == f32w_nw(S), "waves per workgroup");
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_all[];

    const int tid = (int)threadIdx.x;
    const int lane = tid & 63;
    const int piece = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wg = blockIdx.x;
    const WorkItem w = work_item(wg, a.n_items); /* which (dongle, group of 8 channels), placed by XCD */
    const int item = w.item, split = w.split;
    if (split >= a.splits) return;
    const int d = a.item_dev[item], ch0 = a.item_group[item] * 8;
    const DevConst dev = a.dev[d];
    if (dev.disabled) return; /* workgroup-uniform, in front of every barrier */
    const long hop_bytes = a.hop_bytes;

    const TileRange g = tile_range(a.row0, a.first_row, a.ring_rows, a.n_hops);
    const int shift = g.shift, tiles_total = g.tiles_total, ring_tiles = g.ring_tiles, ring_tiles16 = g.ring_tiles16, ptile0 = g.ptile0;
    const Share sh = split_share(tiles_total, a.splits, split);
    const int t_begin = sh.begin, t_end = sh.end;
    if (t_begin >= t_end) return;

    /* the span of this dongle, from the aligned origin at or in front of its first byte, moved on to the window segment of this launch */
    const uint8_t* span = a.iq + (long)d * a.iq_stride;
    const int mis = AL8 ? (int)(reinterpret_cast<uintptr_t>(span) & 15) : 0; /* 0 or 8 (even hops: the span starts on 16 bytes, airband_hip_process_device checks) */
    const uint8_t* src = span - mis + (long)a.seg * (8 * S);
    const long span_end = f32w_span_end(a.n_hops, hop_bytes, S, mis);
    uint8_t* const image = lds_all;
    float4* exch = reinterpret_cast<float4*>(lds_all + f32w_image_bytes(S)); /* [tile parity][NW - 1][64] partial sums on their way to the finishing wave */
    const int fin = wg & (NW - 1);

    /* ---- B fragments: KW registers, resident.  The table is linear in the contraction index: [segment][piece][MFMA][lane] ---- */
    const float* btab = a.btab + (((long)a.item_bset[item] * a.n_seg + a.seg) * NW + piece) * KW * 64 + lane;
    float b[KW];
#pragma unroll
    for (int s = 0; s < KW; s++) b[s] = btab[s * 64];

    const int col = lane & 15, row_l = lane & 15, grp = lane >> 4;
    const int ch = ch0 + (col >> 1);
    const bool ch_valid = ch < dev.n_ch;
    const int slot = a.ext_to_slot[dev.chan_base + (ch_valid ? ch : 0)];
    const unsigned ch_flags = a.cc[slot].flags;
    const bool want_iq = ch_valid && ((ch_flags & AB_F_RAW_IQ) != 0);
    const bool want_mag = !(ch_flags & AB_F_NFM); /* NFM channels: stage 2 recomputes |bin| from the raw I/Q */
    const long slot_base = ab_tile_base(slot, ring_tiles);
    const bool store_lane = !(col & 1) && ch_valid;
    const long lane_off = slot_base + ab_tile_off(grp * 4);
    float* const mag_lane = a.mag + lane_off;
    float2* const iq_lane = a.iq_bins + lane_off;
    constexpr long TILE16_PITCH = (long)TILE_HOPS * AB_SLOT_BLOCK;
    const float scale = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(dev.scale)));

    /* the lane's fragment reads: one base, the reads 64 bytes apart (immediates).  A tile is 16 hops, so the row's delta is the same in every tile */
    const int delta_l = AL8 ? f32w_delta((long)row_l - shift, hop_bytes, mis) : 0;
    const uint8_t* const abase = image + f32w_frag(S, NW, row_l, delta_l, piece, grp, 0);
    static_assert(f32w_frag(S, NW, 0, 0, 0, 0, 1) - f32w_frag(S, NW, 0, 0, 0, 0, 0) == 64, "fragment reads are 64 bytes apart");

    /* ---- staging: registers one tile ahead.  Step i: thread `tid` fetches piece tid % NPR of row RPI i + tid / NPR; AL8: the first sixteen threads also fetch
     * the extra piece of row `tid` ---- */
    v4u stage[MAX_LD];
    const int my_row = tid / NPR, my_col = tid % NPR; /* (powers of two) */
    auto fetch = [&](int row, int pc, long hop0) {
        int nb;
        const long so = f32w_src(row, pc, hop0, hop_bytes, mis, span_end, &nb);
        if (AL8 && nb == 8) { /* the span's last piece, half inside: nothing is read past the span */
            const v2u lo = *reinterpret_cast<const v2u*>(src + so);
            return (v4u){lo.x, lo.y, 0u, 0u};
        }
        return *reinterpret_cast<const v4u*>(src + so);
    };
    auto load_tile = [&](int t) {
        const long hop0 = (long)t * TILE_HOPS - shift;
#pragma unroll
        for (int i = 0; i < ROW_STEPS; i++) stage[i] = fetch(i * RPI + my_row, my_col, hop0);
        if (AL8) {
            if (tid < TILE_HOPS) stage[MAX_LD - 1] = fetch(tid, NPR, hop0);
        }
    };
    auto park_tile = [&]() {
#pragma unroll
        for (int i = 0; i < ROW_STEPS; i++) *reinterpret_cast<v4u*>(image + f32w_park(S, i * RPI + my_row, my_col)) = stage[i];
        if (AL8) {
            if (tid < TILE_HOPS) *reinterpret_cast<v4u*>(image + f32w_park(S, tid, NPR)) = stage[MAX_LD - 1];
        }
    };
    auto frag = [&](const uint8_t* p) { /* four consecutive stream values of the lane's hop */
        if (!AL8) return *reinterpret_cast<const v4f*>(p);
        const v2f lo = *reinterpret_cast<const v2f*>(p), hi = *reinterpret_cast<const v2f*>(p + 8);
        return (v4f){lo.x, lo.y, hi.x, hi.y};
    };
    auto pair_swap = [&](float v) { return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, true)); };

    load_tile(t_begin);
    park_tile();
    for (int t = t_begin; t < t_end; t++) {
        __syncthreads(); /* the image of tile t is whole */
        if (t + 1 < t_end) load_tile(t + 1); /* flies under this tile's MFMAs */
        /* two accumulators, A fragments three reads ahead of their MFMAs behind scheduling fences: channelizer_f32.hip explains both */
        v4f acc = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = {0.0f, 0.0f, 0.0f, 0.0f};
        constexpr int AHEAD = 3;
        v4f av[AHEAD + 1];
#pragma unroll
        for (int j = 0; j < AHEAD && j < READS; j++) av[j] = frag(abase + 64 * j);
#pragma unroll
        for (int j = 0; j < READS; j++) {
            if (j + AHEAD < READS) av[(j + AHEAD) % (AHEAD + 1)] = frag(abase + 64 * (j + AHEAD));
            const v4f x = av[j % (AHEAD + 1)];
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x.x, b[4 * j + 0], acc, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.y, b[4 * j + 1], acc1, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x.z, b[4 * j + 2], acc, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.w, b[4 * j + 3], acc1, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        acc += acc1;
        float4* ex = f32_exchange_put<NW>(exch, t, piece, fin, lane, acc);
        __syncthreads(); /* every wave has read the image; the partial sums are in place */
        if (t + 1 < t_end) park_tile();
        if (piece != fin) continue;
        float val[4] = {acc[0], acc[1], acc[2], acc[3]};
        f32_exchange_sum<NW>(ex, lane, val);
        if (a.n_seg > 1) { /* (launch-uniform) window segments: whole-wave 1 KiB rows of partial sums, one per (work item, tile) */
            float4* row = a.partial + ((long)item * tiles_total + t) * 64 + lane;
            if (a.seg > 0) {
                const float4 o = *row;
                val[0] += o.x; val[1] += o.y; val[2] += o.z; val[3] += o.w;
            }
            if (a.seg + 1 < a.n_seg) {
                *row = make_float4(val[0], val[1], val[2], val[3]);
                continue;
            }
        }
        float im4[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            val[r] *= scale;
            im4[r] = pair_swap(val[r]);
        }
        const bool whole_tile = t * TILE_HOPS - shift >= 0 && t * TILE_HOPS - shift + TILE_HOPS <= a.n_hops; /* wave-uniform */
        int pt = ptile0 + t;
        pt = pt >= ring_tiles16 ? pt - ring_tiles16 : pt;
        if (__builtin_expect(whole_tile, 1)) {
            if (store_lane) {
                const long toff = (long)pt * TILE16_PITCH;
                if (want_mag) {
                    v4f m;
#pragma unroll
                    for (int r = 0; r < 4; r++) m[r] = __builtin_amdgcn_sqrtf(val[r] * val[r] + im4[r] * im4[r]); /* v_sqrt_f32, 1 ulp: stage 1 is tolerance-bound */
                    *reinterpret_cast<v4f*>(mag_lane + toff) = m;
                }
                if (want_iq) {
                    v4f qa = {val[0], im4[0], val[1], im4[1]}, qb = {val[2], im4[2], val[3], im4[3]};
                    v4f* q = reinterpret_cast<v4f*>(iq_lane + toff);
                    q[0] = qa;
                    q[1] = qb;
                }
            }
            continue;
        }
        if (store_lane) { /* first / last tile of a batch: hops outside [0, n_hops) are computed and dropped */
            const long off = slot_base + ab_tile_off(pt * TILE_HOPS + grp * 4);
            const int hop_first = t * TILE_HOPS - shift + grp * 4;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int hop = hop_first + r;
                if (hop >= 0 && hop < a.n_hops) {
                    if (want_mag) a.mag[off + r] = __builtin_amdgcn_sqrtf(val[r] * val[r] + im4[r] * im4[r]);
                    if (want_iq) a.iq_bins[off + r] = make_float2(val[r], im4[r]);
                }
            }
        }
    }
}

template <int S, int NW, bool AL8>
void launch_one(const F32Args& a, hipStream_t stream) {
    const long groups = (long)a.n_items * a.splits;
    const size_t lds = (size_t)f32w_lds_total(S, NW);
    static_assert(F32W_LDS_MAX == CU_LDS_BYTES, "the plans are cut to the LDS that opt_in_big_lds() asks for");
    static std::atomic<bool> big_lds[BIG_LDS_DEVICES]; /* (per kernel variant) */
    opt_in_big_lds(reinterpret_cast<const void*>(&channelizer_f32_wide_kernel<S, NW, AL8>), lds, big_lds);
    hipLaunchKernelGGL((channelizer_f32_wide_kernel<S, NW, AL8>), dim3((unsigned)groups), dim3(64 * NW), lds, stream, a);
}

template <int S, int NW>
void launch_seg(const F32Args& a, hipStream_t stream) {
    if (a.hop_bytes & 8) launch_one<S, NW, true>(a, stream);
    else launch_one<S, NW, false>(a, stream);
}

}  // namespace

int f32_wide_seg_size(int fft_size) {
    const int n = f32w_plan_segments(fft_size);
    return n > 0 ? fft_size / n : 0;
}

int f32_wide_plan(int fft_size, int hop_samples, int* segments, int* lds_bytes) {
    if (fft_size != 256 && fft_size != 512 && fft_size != 1024 && fft_size != 2048 && fft_size != 4096 && fft_size != 8192) return -1;
    if (hop_samples < 8 || f32_supported(fft_size, hop_samples, AIRBAND_SFMT_F32)) return -1; /* the ordinary kernel's shapes stay its own */
    const int n = f32w_plan_segments(fft_size);
    if (n <= 0) return 0;
    const int S = fft_size / n;
    if (segments) *segments = n;
    if (lds_bytes) *lds_bytes = f32w_lds_total(S, f32w_nw(S));
    return n;
}

void launch_channelizer_f32_wide(const F32Args& a0, hipStream_t stream) {
    F32Args a = a0;
    a.n_seg = f32w_plan_segments(a0.fft_size);
    const int S = a0.fft_size / a.n_seg;
    if (a.n_seg == 1) a.partial = nullptr;
    for (int seg = 0; seg < a.n_seg; seg++) {
        a.seg = seg;
        if (S == 256) launch_seg<256, 4>(a, stream);
        else if (S == 512) launch_seg<512, 4>(a, stream);
        else launch_seg<1024, 8>(a, stream);
    }
}

}  // namespace airband
