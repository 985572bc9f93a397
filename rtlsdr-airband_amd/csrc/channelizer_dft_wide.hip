/* csrc/channelizer_dft_wide.hip -- the int8 matrix-core channelizer (channelizer_dft.hip) for hops beyond its contiguous staging: every SoapySDR-class
 * device above ~4 MS/s (CS16 at 6 - 10 MS/s: hops of 1 500 - 5 000 bytes; CS8 at 8 - 20 MS/s), AIRBAND_HIP_FLAG_WIDE_HOPS handles only.
 *
 * The arithmetic is channelizer_dft.hip's, unchanged: the same coefficient tables (three balanced base-256 digits), the same v_mfma_i32_16x16x64_i8 loop, the
 * same CS16 plane split, window pieces and epilogue; a tile is still 16 hops x 16 columns aligned to the rings' row tiles.  What differs is the staging.
 * channelizer_dft.hip keeps ONE contiguous image of a tile's stream, 15 hops + one window: 77 KB at hops of 5 000 bytes -- of which the reference reads the
 * window's 2 048 bytes of every hop and nothing else (src/rtl_airband.cpp:402-455, :669).  Here each of the tile's 16 hops is staged as a ROW:
 *
 *   row r of a tile = PITCH = window + 16 bytes of stream from the aligned 16-byte piece at or in front of hop r's first byte.
 *
 * The 16 rows lie back to back, so a tile's image is 16 x PITCH contiguous LDS bytes and the transfer is ceil(16 PITCH / 1024) global_load_lds of width 16 with
 * EVERY lane active: the destination is lane-linear (instruction i, lane l -> image byte o = 1024 i + 16 l), the source is the lane's own -- row o / PITCH, byte
 * o % PITCH of that row (PITCH is a compile-time constant: a multiply-high).  Per-lane source addresses run at the full rate (row gathers, MI355X_MICROARCH.md);
 * an instruction spans at most two rows at these pitches.  Where hop >= window the kernel reads the windows and skips what lies between them (CS16 at 10 MS/s,
 * WAVE_RATE 8000: 41 % of the stream); where 1 024 < hop < window the rows overlap and the overlap is fetched again, out of L2.
 *
 * A row's first byte sits delta_r = (row start) & 15 bytes into its image; delta_r differs from row to row (hops that are not multiples of 16 bytes), so it is
 * the LANE's (row = lane & 15), recomputed per tile, and the AL = 16 / 8 / 4 / 2 fragment readers of dft_common.h take it as part of their address.
 *
 * Banks.  An A fragment read is lane l -> row (l & 15), 16 bytes at k-chunk (l >> 4).  ds_read_b128 serves four groups of 16 lanes, each eight rows of one
 * k-chunk and eight of the next, and its bank is (address / 4) mod 64: sixteen 16-byte columns per 256 bytes.  PITCH / 16 = window / 16 + 1 is ODD (the window is
 * a multiple of 512 bytes), so the 16 rows of a chunk fall on 16 different columns -- with PITCH = window they would all fall on ONE (16-way).  The two half
 * sets of a group are one column apart and meet in exactly one column (A = {0-3, 12-15}, B = {4-11} + 1 share 12): 2-way on one of 16 columns, which is what
 * the contiguous image has at hops of 320 bytes; no odd multiple does better (B is A's complement shifted by one column, and no 8-set equals its shift).  The 16
 * bytes of padding are the very bytes an unaligned row needs anyway.
 *
 * Buffers: two tile images, one tile ahead, the wait counts of channelizer_dft.hip's two-buffer path (everything younger than a tile's transfer = the output
 * stores issued since).  Window pieces (fft_size 1024 ...): wave 0 issues the transfers, one barrier hands a tile over, a second orders the partial sums.
 * LDS: 2 x roundup(16 PITCH, 1 KiB) + the exchange area -- independent of the hop (kernels.h, dft_wide_lds_bytes).
 *
 * Segments (SEG = 2, 4: CS16 fft 2048, u8 / s8 fft 4096, CS16 fft 4096 -- windows of 4 - 16 KiB, whose two whole images would be 258 - 514 KiB).  Every wave reads
 * only its own piece of a row, so every piece is cut into SEG equal segments along k and an image holds, for the 16 hops and all NP pieces, ONE segment of
 * S = WIN_BYTES / SEG bytes: 16 x NP sub-rows of S + 16 bytes, piece-major, so that the 16 hops of a piece stay one odd pitch apart (dft_wide_map.h: the layout,
 * and both directions of the address map as functions the host can run -- this file computes no image address of its own).  The two buffers alternate per
 * SEGMENT: while the waves run the MFMAs of segment s of tile t, wave 0 streams in segment s + 1, or segment 0 of tile t + 1; the sums (TileAcc) live across a
 * tile's segments; recombination, the exchange and the stores happen once per tile.  The hand-over is the same wait + one barrier, the proof that a transfer has
 * landed the same count of stores since.  A segment starts a multiple of 16 bytes into its row: delta is the row's, unchanged.  LDS: 136 KiB (CS16 fft 2048), 146 KiB
 * (fft 4096), one workgroup per CU.  SEG = 1 is the kernel above: the same arithmetic, LDS and register counts (the compiled code differs in register numbering and two address instructions).  Not built: SEG > 1 with the AL = 2 reader (u8 / s8 fft 4096 at hops of
 * an odd number of samples) -- with the sums live across the staging loop it spills 29 registers; dft_wide_plan() keeps that shape on the wavefront FFT.
 *
 * From mfma_front.h: work_item(), tile_range(), split_share(), opt_in_big_lds(); from dft_common.h: TileAcc, recombine(), digit_value(), piece_sum(), wait_vmcnt_lo(), ab_mfma(), lds_read16(). */
#include <hip/hip_runtime.h>
#include <atomic>
#include <utility>

#include "common.h"
#include "kernels.h"
#include "dft_common.h"

namespace airband {

namespace {

/* s_waitcnt vmcnt(n), n wave-uniform, for this kernel's counts: the output stores since a transfer was issued (0 - 6 in the steady state) */
__device__ __forceinline__ void wait_stores(int n) { wait_vmcnt_lo(n); }

/* f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): the segments of a tile, each with its own compile-time slice of the B fragments */
template <int... I, class F>
__device__ __forceinline__ void each_segment(std::integer_sequence<int, I...>, F&& f) {
    (f(std::integral_constant<int, I>{}), ...);
}

template <bool EDGE_HI_ZERO, int FFT_N, bool S16, int AL, int NP, int SEG>
__global__ __launch_bounds__(64 * NP, NP <= 4 ? 2 : 1) void channelizer_dft_wide_kernel(DftArgs a) {
    constexpr int BPS = S16 ? 2 : 1;
    constexpr int WIN_BYTES = 2 * FFT_N * BPS; /* bytes per window piece */
    constexpr int WIN_ALL = WIN_BYTES * NP;    /* bytes per window       */
    typedef WideMap<WIN_BYTES, NP, SEG> Map;   /* dft_wide_map.h: the image's layout and both directions of its address map */
    constexpr int BUF = Map::IMAGE;
    constexpr int N_DMA = Map::N_DMA;
    constexpr int KSTEPS = 2 * FFT_N / 64;
    constexpr int KSEG = KSTEPS / SEG;         /* k-steps per segment */
    static_assert(KSTEPS == 16 || KSTEPS == 8, "fft_size 256 or 512 per window piece");
    static_assert(NP == 1 || FFT_N == 512, "window pieces are 512 samples long");
    static_assert(SEG == 1 || (NP > 1 && KSEG >= 4 && KSEG * SEG == KSTEPS), "segments: windows in pieces only, at least four k-steps each");
    constexpr int EDGE = KSTEPS / 8;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_all[];

    const int lane = NP > 1 ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
    const int piece = NP > 1 ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : 0;
    const WorkItem w = work_item((int)blockIdx.x, a.n_items); /* which (dongle, group of 8 channels), placed by XCD (mfma_front.h) */
    const int item = w.item, split = w.split;
    if (split >= a.splits) return;
    const int d = a.item_dev[item], ch0 = a.item_group[item] * 8;
    if (a.dev[d].disabled) return; /* workgroup-uniform, in front of every barrier */
    const long hop_bytes = a.hop_bytes;

    const TileRange g = tile_range(a.row0, a.first_row, a.ring_rows, a.n_hops);
    const int shift = g.shift, tiles_total = g.tiles_total, ring_tiles = g.ring_tiles, ring_tiles16 = g.ring_tiles16, ptile0 = g.ptile0;
    const uint8_t* src = a.iq + (long)d * a.iq_stride;
    /* the transfers move aligned 16-byte pieces: the stream is addressed from the aligned byte at or in front of the span's first one */
    const int mis = (int)(reinterpret_cast<uintptr_t>(src) & 15u);
    src -= mis;
    const Share sh = split_share(tiles_total, a.splits, split);
    const int t_begin = sh.begin, t_end = sh.end;
    if (t_begin >= t_end) return;
    /* bytes of the batch span that may be read, from `src`, in whole 16-byte pieces: the last hop's window and not a byte more (geometry.lookahead_bytes
     * includes the round-up) */
    const long span_end = wide_span_end(a.n_hops, hop_bytes, WIN_ALL, mis);

    /* ---- B fragments, resident for the whole wave ---- */
    const int bset = a.item_bset[item] * NP + piece;
    const v4i* btab = reinterpret_cast<const v4i*>(a.bfrag) + (long)bset * 3 * KSTEPS * 64 + lane;
    v4i b0[KSTEPS], b1[KSTEPS], b2[KSTEPS];
#pragma unroll
    for (int s = 0; s < KSTEPS; s++) {
        b0[s] = btab[(0 * KSTEPS + s) * 64];
        b1[s] = btab[(1 * KSTEPS + s) * 64];
        if (!(EDGE_HI_ZERO && (s < EDGE || s >= KSTEPS - EDGE))) b2[s] = btab[(2 * KSTEPS + s) * 64];
    }
    const int col = lane & 15;
    const double corr = S16 ? a.corr[bset * 16 + col] * 256.0 : a.corr[bset * 16 + col];
    const int ch = ch0 + (col >> 1);
    const DevConst dev = a.dev[d];
    const double unscale = S16 ? a.unscale * (double)dev.scale : a.unscale;
    const bool ch_valid = ch < dev.n_ch;
    const int slot = a.ext_to_slot[dev.chan_base + (ch_valid ? ch : 0)];
    const unsigned ch_flags = a.cc[slot].flags;
    const bool want_iq = ch_valid && ((ch_flags & AB_F_RAW_IQ) != 0);
    const bool want_mag = !(ch_flags & AB_F_NFM);
    const long slot_base = ab_tile_base(slot, ring_tiles);

    typedef __attribute__((address_space(1))) const void* gptr_t;
    typedef __attribute__((address_space(3))) void* lptr_t;
    /* segment `seg` of tile t -> image `buf`: lane l of instruction i fills image byte o = 1024 i + 16 l = byte o % PITCH of sub-row o / PITCH (Map::src: which
     * stream bytes those are, and what stands in for addresses outside the batch span) */
    auto stage = [&](int t, int seg, uint8_t* buf) {
        const long hop0 = (long)t * TILE_HOPS - shift;
#pragma unroll 1 /* (unrolled, the 33 - 66 per-lane addresses of an image are all computed up front and spill the B fragments) */
        for (int i = 0; i < N_DMA; i++) {
            const long so = Map::src((unsigned)(i * WIDE_DMA_BYTES + lane * 16), hop0, hop_bytes, mis, seg, span_end);
            __builtin_amdgcn_global_load_lds((gptr_t)(src + so), (lptr_t)(uintptr_t)(buf + i * WIDE_DMA_BYTES), 16, 0, 0);
        }
    };
    float4* exch = reinterpret_cast<float4*>(lds_all + 2 * BUF); /* partial sums of pieces 1 .. NP-1 on their way to wave 0: [tile parity][piece - 1][lane] */
    /* `stores`: output store instructions issued so far (whole tiles only: fewer than the truth is safe); mark*: what it stood at when the transfer into the
     * buffer was issued -- vector-memory operations complete in issue order, so "at most stores - mark outstanding" proves that transfer has landed */
    int stores = 0, mark0 = 0, mark1 = 0;
    if (piece == 0) stage(t_begin, 0, lds_all);

    const int row_l = lane & 15, grp = lane >> 4;
    const int k_tile = ((__ballot(!(col & 1) && ch_valid && want_mag) != 0ull) ? 1 : 0) + ((__ballot(!(col & 1) && ch_valid && want_iq) != 0ull) ? 2 : 0);

    const Recombine rc = recombine(unscale, corr, a.sfmt);
    const int flipmask = rc.flipmask;

    /* LDS -> MFMA for the 16 hops of tile t, k-steps [SG x KSEG, (SG + 1) x KSEG) of the wave's piece out of the image of segment SG: the lane's row, delta_r
     * bytes in.  The first segment starts the sums, the others add to them */
    auto seg_mfma = [&](const uint8_t* buf, int t, TileAcc& A, auto seg_c) {
        constexpr int SG = decltype(seg_c)::value, K0 = SG * KSEG;
        const int delta = AL >= 16 ? 0 : wide_delta((long)t * TILE_HOPS - shift + row_l, hop_bytes, mis);
        const uint8_t* arow = buf + Map::frag(row_l, piece, SG, SG * Map::S) + delta + grp * (S16 ? 32 : 16);
        if (SG == 0) { A.a0 = (v4i){0, 0, 0, 0}; A.a1 = (v4i){0, 0, 0, 0}; A.a2 = (v4i){0, 0, 0, 0}; }
        if (!S16) {
            v4i av[KSEG];
            av[0] = lds_read16<AL>(arow); av[1] = lds_read16<AL>(arow + 64); av[2] = lds_read16<AL>(arow + 128); av[3] = lds_read16<AL>(arow + 192);
#pragma unroll
            for (int i = 0; i < KSEG; i++) {
                const int s = K0 + i; /* the k-step of the piece (compile-time once unrolled): which B fragment, which edge */
                if ((i & 1) == 0 && i + 4 < KSEG) { /* fetched four k-steps ahead of the MFMAs that consume them */
                    av[i + 4] = lds_read16<AL>(arow + (i + 4) * 64);
                    av[i + 5] = lds_read16<AL>(arow + (i + 5) * 64);
                }
                v4i x = av[i];
                x.x ^= flipmask; x.y ^= flipmask; x.z ^= flipmask; x.w ^= flipmask; /* u8 -> b - 128 as int8; s8 is int8 already */
                A.a0 = ab_mfma(x, b0[s], A.a0);
                A.a1 = ab_mfma(x, b1[s], A.a1);
                if (!(EDGE_HI_ZERO && (s < EDGE || s >= KSTEPS - EDGE))) A.a2 = ab_mfma(x, b2[s], A.a2);
                if (i & 1) __builtin_amdgcn_sched_barrier(0);
            }
        } else {
            /* CS16: plane k-step s of the lane = 16 plane bytes = 8 samples x (I, Q) = 32 raw bytes [Ilo Ihi Qlo Qhi] x 8, pulled apart with v_perm_b32 */
            if (SG == 0) { A.h0 = (v4i){0, 0, 0, 0}; A.h1 = (v4i){0, 0, 0, 0}; A.h2 = (v4i){0, 0, 0, 0}; }
            v4i ra[2], rb[2];
            ra[0] = lds_read16<AL>(arow);
            rb[0] = lds_read16<AL>(arow + 16);
#pragma unroll
            for (int i = 0; i < KSEG; i++) {
                const int s = K0 + i;
                if (i + 1 < KSEG) {
                    ra[(i + 1) & 1] = lds_read16<AL>(arow + (i + 1) * 128);
                    rb[(i + 1) & 1] = lds_read16<AL>(arow + (i + 1) * 128 + 16);
                }
                const v4i p = ra[i & 1], q = rb[i & 1];
                v4i lo, hi;
                lo.x = (int)__builtin_amdgcn_perm((unsigned)p.y, (unsigned)p.x, 0x06040200u); hi.x = (int)__builtin_amdgcn_perm((unsigned)p.y, (unsigned)p.x, 0x07050301u);
                lo.y = (int)__builtin_amdgcn_perm((unsigned)p.w, (unsigned)p.z, 0x06040200u); hi.y = (int)__builtin_amdgcn_perm((unsigned)p.w, (unsigned)p.z, 0x07050301u);
                lo.z = (int)__builtin_amdgcn_perm((unsigned)q.y, (unsigned)q.x, 0x06040200u); hi.z = (int)__builtin_amdgcn_perm((unsigned)q.y, (unsigned)q.x, 0x07050301u);
                lo.w = (int)__builtin_amdgcn_perm((unsigned)q.w, (unsigned)q.z, 0x06040200u); hi.w = (int)__builtin_amdgcn_perm((unsigned)q.w, (unsigned)q.z, 0x07050301u);
                lo.x ^= 0x80808080; lo.y ^= 0x80808080; lo.z ^= 0x80808080; lo.w ^= 0x80808080; /* unsigned low byte -> lo - 128 as int8 */
                A.a0 = ab_mfma(lo, b0[s], A.a0);
                A.h0 = ab_mfma(hi, b0[s], A.h0);
                A.a1 = ab_mfma(lo, b1[s], A.a1);
                A.h1 = ab_mfma(hi, b1[s], A.h1);
                if (!(EDGE_HI_ZERO && (s < EDGE || s >= KSTEPS - EDGE))) {
                    A.a2 = ab_mfma(lo, b2[s], A.a2);
                    A.h2 = ab_mfma(hi, b2[s], A.h2);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
    /* digit sums -> the lane's four values (hops grp * 4 .. + 3 of column col), in single precision: every accumulator is an exact integer below 2^24 */
    auto tile_value = [&](const TileAcc& A, int r) { return digit_value<S16>(A, rc, r); };
    auto pair_swap = [&](float v) { return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, true)); };
    typedef float v4f __attribute__((ext_vector_type(4)));
    const bool store_lane = !(col & 1) && ch_valid;
    const long lane_off = slot_base + ab_tile_off(grp * 4);
    float* const mag_lane = a.mag + lane_off;
    float2* const iq_lane = a.iq_bins + lane_off;
    constexpr long TILE16_PITCH = (long)TILE_HOPS * AB_SLOT_BLOCK;
    /* values of tile t -> rings: lane pairs (2 ch, 2 ch + 1) hold (re, im) of the same hop; even lanes write 4 consecutive rows of their slot */
    auto tile_store = [&](int t, const float* val) {
        float im4[4];
#pragma unroll
        for (int r = 0; r < 4; r++) im4[r] = pair_swap(val[r]);
        const bool whole_tile = t * TILE_HOPS - shift >= 0 && t * TILE_HOPS - shift + TILE_HOPS <= a.n_hops;
        int pt = ptile0 + t;
        pt = pt >= ring_tiles16 ? pt - ring_tiles16 : pt;
        if (__builtin_expect(whole_tile, 1)) {
            stores += k_tile;
            if (store_lane) {
                const long toff = (long)pt * TILE16_PITCH;
                if (want_mag) {
                    v4f m;
#pragma unroll
                    for (int r = 0; r < 4; r++) m[r] = __builtin_amdgcn_sqrtf(val[r] * val[r] + im4[r] * im4[r]);
                    *reinterpret_cast<v4f*>(mag_lane + toff) = m;
                }
                if (want_iq) {
                    v4f qa = {val[0], im4[0], val[1], im4[1]}, qb = {val[2], im4[2], val[3], im4[3]};
                    asm volatile("" : "+v"(qa), "+v"(qb));
                    v4f* q = reinterpret_cast<v4f*>(iq_lane + toff);
                    q[0] = qa;
                    q[1] = qb;
                }
            }
            return;
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
    };

    int cur = 0;
    for (int t = t_begin; t < t_end; t++) {
        TileAcc now; /* lives across the segments of the tile */
        each_segment(std::make_integer_sequence<int, SEG>{}, [&](auto seg_c) {
            constexpr int SG = decltype(seg_c)::value;
            uint8_t* buf = lds_all + cur * BUF;
            /* NP > 1: wave 0 runs the transfers and the waits; the barrier hands the image (segment SG of tile t) to the other waves and tells wave 0 that they are
             * done with the buffer the next transfer overwrites (they read it one image ago) */
            if (piece == 0) wait_stores(stores - (cur ? mark1 : mark0)); /* the image's bytes have landed: younger than its transfer are only the stores since */
            if (NP > 1) __syncthreads();
            if (piece == 0 && (SG + 1 < SEG || t + 1 < t_end)) { /* the next image -- the tile's next segment, or the next tile's first -- streams in under these MFMAs */
                stage(SG + 1 < SEG ? t : t + 1, SG + 1 < SEG ? SG + 1 : 0, lds_all + (cur ^ 1) * BUF);
                if (cur) mark0 = stores;
                else mark1 = stores;
            }
            seg_mfma(buf, t, now, seg_c);
            cur ^= 1;
        });
        float val[4];
#pragma unroll
        for (int r = 0; r < 4; r++) val[r] = tile_value(now, r);
        if (NP > 1) {
            if (piece > 0) exch[((t & 1) * (NP - 1) + (piece - 1)) * 64 + lane] = make_float4(val[0], val[1], val[2], val[3]);
            __syncthreads();
            if (piece == 0) {
                piece_sum<NP>(exch, t, lane, val);
                tile_store(t, val);
            }
        } else {
            tile_store(t, val);
        }
    }
}

template <int FFT_N, bool S16, int AL, int NP, int SEG>
void launch_al(const DftArgs& a, hipStream_t stream) {
    static_assert(SEG > 0 && wide_lds_total(2 * FFT_N * (S16 ? 2 : 1), NP, SEG) <= WIDE_LDS_MAX, "a shape without a plan has no kernel");
    const long groups = (long)a.n_items * a.splits;
    const size_t lds = (size_t)wide_lds_total(2 * FFT_N * (S16 ? 2 : 1), NP, SEG) + (size_t)(a.extra_lds > 0 ? a.extra_lds : 0);
    static_assert(WIDE_LDS_MAX == CU_LDS_BYTES, "the plans are cut to the LDS that opt_in_big_lds() asks for");
    static std::atomic<bool> big_lds[2][BIG_LDS_DEVICES]; /* (per kernel variant: this instantiation x EDGE_HI_ZERO) */
    const int e = a.edge_hi_zero ? 1 : 0;
    const void* fn = e ? reinterpret_cast<const void*>(&channelizer_dft_wide_kernel<true, FFT_N, S16, AL, NP, SEG>)
                       : reinterpret_cast<const void*>(&channelizer_dft_wide_kernel<false, FFT_N, S16, AL, NP, SEG>);
    opt_in_big_lds(fn, lds, big_lds[e]);
    if (e)
        hipLaunchKernelGGL((channelizer_dft_wide_kernel<true, FFT_N, S16, AL, NP, SEG>), dim3((unsigned)groups), dim3(64 * NP), lds, stream, a);
    else
        hipLaunchKernelGGL((channelizer_dft_wide_kernel<false, FFT_N, S16, AL, NP, SEG>), dim3((unsigned)groups), dim3(64 * NP), lds, stream, a);
}

/* the shape's segments are the plan's (dft_wide_map.h), at compile time: the kernel a handle launches cannot disagree with the LDS dft_wide_plan() promised it */
template <int FFT_N, bool S16, int NP>
void launch_generic(const DftArgs& a, hipStream_t stream) {
    constexpr int SEG = wide_plan_segments(2 * FFT_N * (S16 ? 2 : 1), NP);
    if ((a.hop_bytes & 15) == 0) return launch_al<FFT_N, S16, 16, NP, SEG>(a, stream);
    if ((a.hop_bytes & 7) == 0) return launch_al<FFT_N, S16, 8, NP, SEG>(a, stream);
    if ((a.hop_bytes & 3) == 0) return launch_al<FFT_N, S16, 4, NP, SEG>(a, stream);
    /* u8 / s8 hops of an odd number of samples -- whole windows only: with segments, whose sums live across the staging, this reader's five dwords per fragment
     * spill 29 registers (fft 4096), and a spilling variant is not shipped: dft_wide_plan() keeps that shape off this kernel */
    if constexpr (!S16 && SEG == 1) launch_al<FFT_N, false, 2, NP, SEG>(a, stream);
}

}  // namespace

/* Which hops are this file's business (AIRBAND_HIP_FLAG_WIDE_HOPS handles): exactly those dft_supported() refuses for their LENGTH -- u8 / s8 above 1 024 bytes,
 * CS16 above 1 280 -- at any even length (CS16: whole samples, multiples of 4 bytes).  dft_wide_lds(): the LDS of two WHOLE tile images and the exchange area,
 * 16 x (window + 16) bytes per image whatever the hop: u8 / s8 up to fft_size 2048 and CS16 up to 1024 fit a CU's 160 KiB (two buffers of 65 KiB), nothing larger
 * does -- dft_wide_plan() below then cuts the pieces into segments.
 * Layout rule for 1 024 < hop < window (CS16 hops of 1 500 bytes at fft 512, everything from fft 1024 up): rows as well.  A contiguous image would be
 * 15 hop + window bytes there, less than the rows' 16 x (window + 16) -- 24.5 against 32.3 KiB at CS16 hops of 1 500 bytes -- but it is a second staging path for
 * one kernel and its LDS grows with the hop; the rows' LDS does not depend on the hop, so ONE bound serves every rate, and what neighbouring rows fetch twice
 * comes out of L2, not out of memory. */
int dft_wide_lds(int fft_size, int hop_bytes, int sfmt) {
    if (fft_size < 256 || fft_size > 8192 || (fft_size & (fft_size - 1))) return -1;
    const bool s16 = sfmt == AIRBAND_SFMT_S16;
    if (!s16 && sfmt != AIRBAND_SFMT_U8 && sfmt != AIRBAND_SFMT_S8) return -1;
    if (hop_bytes <= (s16 ? 1280 : 1024) || (hop_bytes % (s16 ? 4 : 2)) != 0) return -1;
    const int np = fft_size > 512 ? fft_size / 512 : 1;
    const long win_all = 2L * fft_size * (s16 ? 2 : 1);
    if (win_all > (1 << 20)) return -1;
    return dft_wide_lds_bytes((int)win_all, np);
}

int dft_wide_plan(int fft_size, int hop_bytes, int sfmt, int* lds_bytes, bool* spills) {
    if (spills) *spills = false;
    if (dft_wide_lds(fft_size, hop_bytes, sfmt) < 0) return -1;
    const int np = fft_size > 512 ? fft_size / 512 : 1;
    const int win_bytes = 2 * (fft_size > 512 ? 512 : fft_size) * (sfmt == AIRBAND_SFMT_S16 ? 2 : 1);
    int seg = wide_plan_segments(win_bytes, np);
    if (seg > 1 && (hop_bytes & 3) != 0) { /* no segmented kernel for u8 / s8 hops of an odd number of samples (launch_generic) */
        seg = 0;
        if (spills) *spills = true;
    }
    if (seg > 0 && lds_bytes) *lds_bytes = wide_lds_total(win_bytes, np, seg);
    return seg;
}

void launch_channelizer_dft_wide(const DftArgs& a0, hipStream_t stream) {
    DftArgs a = a0;
    const bool s16 = a.sfmt == AIRBAND_SFMT_S16;
    a.np_total = a0.fft_size > 512 ? a0.fft_size / 512 : 1;
    a.piece0 = 0;
    a.partial = nullptr;
    switch (a0.fft_size) {
    case 256: return s16 ? launch_generic<256, true, 1>(a, stream) : launch_generic<256, false, 1>(a, stream);
    case 512: return s16 ? launch_generic<512, true, 1>(a, stream) : launch_generic<512, false, 1>(a, stream);
    case 1024: return s16 ? launch_generic<512, true, 2>(a, stream) : launch_generic<512, false, 2>(a, stream);
    case 2048: return s16 ? launch_generic<512, true, 4>(a, stream) : launch_generic<512, false, 4>(a, stream);
    case 4096: return s16 ? launch_generic<512, true, 8>(a, stream) : launch_generic<512, false, 8>(a, stream);
    default: return; /* (fft_size 8192 has no plan: prep_channelizer() never sends it here) */
    }
}

}  // namespace airband
