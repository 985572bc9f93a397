/* csrc/f32_wide_map.h -- the address map of the CF32 wide-hop staging (channelizer_f32_wide.hip): where a staged 16-byte piece comes from in the stream, where it
 * is parked in LDS, and which LDS bytes a fragment read takes.  Plain integer arithmetic, host and device, as dft_wide_map.h: the kernel calls these functions and
 * nothing else computes the addresses, so what a host compiler checks here (tests/test_wide_hops_f32.py, tests/host_f32_wide_map.cpp) is what the kernel does.
 *
 * A tile is 16 hops.  The image holds one ROW per hop: the S window samples (8 S bytes) a launch contracts, staged from the aligned 16-byte piece at or in front
 * of the row's first byte.  Hops of an even number of samples are whole 16-byte pieces: a row is S / 2 pieces and starts on one.  Hops of an odd number of samples
 * are 8 mod 16 bytes long: rows start alternately 0 and 8 bytes (`delta`) behind an aligned piece, a row is staged as S / 2 + 1 pieces, and a fragment is read as
 * two 8-byte halves.  Since a tile is 16 hops a row's delta is the same in every tile of a launch.
 *
 * The row pitch is 8 S + 16 bytes whatever the hop: an odd number of 16-byte units (S is a power of two >= 128), so the 16 rows of a fragment read fall in 16
 * different bank groups, and the 16 spare bytes are the odd rows' extra piece. */
#ifndef AIRBAND_CSRC_F32_WIDE_MAP_H
#define AIRBAND_CSRC_F32_WIDE_MAP_H

#if defined(__HIPCC__)
#define AB_F32W_HD __host__ __device__ __forceinline__ constexpr
#else
#define AB_F32W_HD inline constexpr
#endif

namespace airband {

constexpr int F32W_TILE_HOPS = 16;
constexpr int F32W_LDS_MAX = 160 * 1024; /* a CU's 163 840 bytes */

/* S = window samples staged at a time (one launch), NW = waves per workgroup = pieces of the contraction index */
constexpr int f32w_pitch(int S) { return 8 * S + 16; }
constexpr int f32w_image_bytes(int S) { return F32W_TILE_HOPS * f32w_pitch(S); }
/* ONE image (the tile after it waits in registers) + the exchange area of the pieces' partial sums ([tile parity][NW - 1][64 lanes] float4) */
constexpr int f32w_lds_total(int S, int NW) { return f32w_image_bytes(S) + 2 * (NW - 1) * 64 * 16; }
/* 16-byte pieces staged per row */
constexpr int f32w_row_pieces(int S, bool odd_hop) { return S / 2 + (odd_hop ? 1 : 0); }
/* waves per workgroup for a staged segment of S samples (kernels.h f32_nw() of the fft size whose window S is) */
constexpr int f32w_nw(int S) { return S <= 512 ? 4 : 8; }

/* The plan: the smallest power-of-two number of equal window segments whose staging fits a CU's LDS. */
constexpr int f32w_plan_segments(int fft_size) {
    int seg = 1;
    while (fft_size / seg >= 128 && f32w_lds_total(fft_size / seg, f32w_nw(fft_size / seg)) > F32W_LDS_MAX) seg *= 2;
    return fft_size / seg >= 128 ? seg : 0;
}

/* `mis`: offset of the span's first byte from the aligned 16-byte piece at or in front of it (0, or 8 with odd hops).  All stream offsets below count from that
 * aligned ORIGIN (span start - mis). */
AB_F32W_HD long f32w_row_origin(long hop, long hop_bytes, int mis) { return (hop * hop_bytes + mis) & ~15L; } /* (two's complement: rounds down for hops < 0 too) */
AB_F32W_HD int f32w_delta(long hop, long hop_bytes, int mis) { return (int)((hop * hop_bytes + mis) & 15L); }
/* end of the bytes a launch may read, from the origin: the last hop's staged samples and not a byte more (a multiple of 8; of 16 with even hops) */
AB_F32W_HD long f32w_span_end(int n_hops, long hop_bytes, int S, int mis) { return (long)(n_hops - 1) * hop_bytes + 8L * S + mis; }

/* Source of piece `col` of row `row` of the tile whose first hop is hop0 (negative in a batch's first tile): offset from the origin; *n_bytes = 16, or 8 where
 * only the piece's first half lies inside the span (odd hops, the span's last piece).  Pieces past the span re-read its last piece, pieces in front of it its
 * first: they feed hops outside [0, n_hops), which are never stored, and odd rows' unused halves. */
AB_F32W_HD long f32w_src(int row, int col, long hop0, long hop_bytes, int mis, long span_end, int* n_bytes) {
    long so = f32w_row_origin(hop0 + row, hop_bytes, mis) + 16L * col;
    const long last = (span_end - 1) & ~15L; /* the aligned piece that holds the span's last byte */
    if (so > last) so = last;
    if (so < 0) so = 0;
    *n_bytes = so + 16 > span_end ? 8 : 16;
    return so;
}

/* LDS byte where that piece is parked */
AB_F32W_HD int f32w_park(int S, int row, int col) { return row * f32w_pitch(S) + 16 * col; }

/* LDS byte of the j-th fragment read (16 bytes = four stream values; two 8-byte halves where delta = 8) of lane group `grp` (lane >> 4) of the wave that owns
 * piece `piece` of the contraction index, for the tile's hop `row` */
AB_F32W_HD int f32w_frag(int S, int NW, int row, int delta, int piece, int grp, int j) { return row * f32w_pitch(S) + delta + piece * (8 * S / NW) + 64 * j + 16 * grp; }

}  // namespace airband
#endif
