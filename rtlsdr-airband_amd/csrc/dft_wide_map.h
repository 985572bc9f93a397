/* csrc/dft_wide_map.h -- the address map of the wide-hop staging (channelizer_dft_wide.hip): where an image byte comes from in the stream, and which image byte
 * a fragment read takes.  Plain integer arithmetic, host and device: the kernel calls these functions and nothing else computes the addresses, so what a host
 * compiler checks here (tests/test_wide_windows.py) is what the kernel does -- the matrix-core channelizer itself cannot be emulated on the host.
 *
 * A tile is 16 hops.  A window is NP pieces of WIN_BYTES (one wavefront each), and every piece is cut into SEG equal segments of S = WIN_BYTES / SEG bytes along k.
 *
 *   SEG = 1: an image holds, per hop, ONE sub-row: the whole window, NP x WIN_BYTES + 16 bytes from the aligned 16-byte piece at or in front of the hop's first byte.
 *   SEG > 1: an image holds, per hop and piece, one sub-row: segment s of that piece, S + 16 bytes from the same aligned origin + piece x WIN_BYTES + s x S.
 *
 * Sub-rows lie back to back, PIECE-major: sub-row (piece j, hop r) is number 16 j + r.  The 16 hops of a piece are then one pitch apart, and the pitch -- a
 * multiple of 512 bytes plus 16 -- is an odd number of 16-byte bank columns: the 16 rows of a k-chunk fall on 16 different columns (hop-major, the rows would be
 * NP pitches apart and share 16 / NP columns).  The 16 bytes of padding are the bytes an unaligned row needs: a segment starts a multiple of 16 bytes into its
 * row, so a row's delta (its first byte's offset from the aligned origin) is the same for every piece and segment. */
#ifndef AIRBAND_CSRC_DFT_WIDE_MAP_H
#define AIRBAND_CSRC_DFT_WIDE_MAP_H

#if defined(__HIPCC__)
#define AB_WIDE_HD __host__ __device__ __forceinline__
#else
#define AB_WIDE_HD inline
#endif

namespace airband {

constexpr int WIDE_TILE_HOPS = 16;
constexpr int WIDE_DMA_BYTES = 1024; /* one transfer: 64 lanes x 16 bytes, lane-linear in the image */

/* the geometry of one (window piece, pieces, segments) shape */
constexpr int wide_n_sub(int np, int seg) { return seg == 1 ? 1 : np; }                                      /* sub-rows per hop */
constexpr int wide_sub_len(int win_bytes, int np, int seg) { return seg == 1 ? win_bytes * np : win_bytes / seg; } /* stream bytes a sub-row serves */
constexpr int wide_sub_pitch(int win_bytes, int np, int seg) { return wide_sub_len(win_bytes, np, seg) + 16; }
constexpr int wide_image_bytes(int win_bytes, int np, int seg) {
    return (WIDE_TILE_HOPS * wide_n_sub(np, seg) * wide_sub_pitch(win_bytes, np, seg) + WIDE_DMA_BYTES - 1) / WIDE_DMA_BYTES * WIDE_DMA_BYTES;
}
/* two images + the exchange area of the pieces' partial sums ([tile parity][piece - 1][64 lanes] float4) */
constexpr int wide_lds_total(int win_bytes, int np, int seg) { return 2 * wide_image_bytes(win_bytes, np, seg) + (np > 1 ? 2 * (np - 1) * 64 * 16 : 0); }

/* The plan: the fewest segments, 1 / 2 / 4, with which the two images and the exchange area fit a CU's LDS (one workgroup per CU then); 0 where none does.
 * Shapes that fit whole (every one up to u8 / s8 fft 2048 and CS16 fft 1024) therefore stay on one segment.  Segments need window pieces (np > 1), and a
 * workgroup is at most eight of them. */
constexpr int WIDE_LDS_MAX = 160 * 1024;
constexpr int wide_plan_segments(int win_bytes, int np) {
    if (np > 8) return 0;
    if (wide_lds_total(win_bytes, np, 1) <= WIDE_LDS_MAX) return 1;
    if (np > 1 && wide_lds_total(win_bytes, np, 2) <= WIDE_LDS_MAX) return 2;
    if (np > 1 && wide_lds_total(win_bytes, np, 4) <= WIDE_LDS_MAX) return 4;
    return 0;
}

/* bytes of the batch span that may be read, from the aligned origin, in whole 16-byte pieces: the last hop's window and not a byte more */
AB_WIDE_HD long wide_span_end(int n_hops, long hop_bytes, int win_all, int mis) { return ((long)(n_hops - 1) * hop_bytes + win_all + mis + 15) & ~15L; }

/* offset of hop `hop`'s first byte from the aligned 16-byte piece at or in front of it (`mis`: the span's own offset from ITS aligned piece) */
AB_WIDE_HD int wide_delta(long hop, long hop_bytes, int mis) { return (int)((hop * hop_bytes + mis) & 15L); }

template <int WIN_BYTES, int NP, int SEG>
struct WideMap {
    static_assert(SEG >= 1 && WIN_BYTES % (16 * SEG) == 0, "segments are whole 16-byte pieces");
    static constexpr int N_SUB = wide_n_sub(NP, SEG);
    static constexpr int S = WIN_BYTES / SEG;
    static constexpr int PITCH = wide_sub_pitch(WIN_BYTES, NP, SEG);
    static constexpr int IMAGE = wide_image_bytes(WIN_BYTES, NP, SEG);
    static constexpr int N_DMA = IMAGE / WIDE_DMA_BYTES;

    /* Transfer i, lane l fills image bytes [o, o + 16), o = 1024 i + 16 l, of segment `seg` of the tile whose first hop is hop0 (negative in a batch's first tile):
     * the offset of their source from the span's aligned origin.  Sources past the span re-read its last 16 bytes, sources in front of it its first: they feed hops
     * outside [0, n_hops), which are never stored, and the padding.  Image bytes behind the last sub-row (up to the image's whole KiB) are read by nobody. */
    static AB_WIDE_HD long src(unsigned o, long hop0, long hop_bytes, int mis, int seg, long span_end) {
        unsigned q = o / (unsigned)PITCH, off = o - q * (unsigned)PITCH;
        if (q > (unsigned)(WIDE_TILE_HOPS * N_SUB - 1)) {
            q = WIDE_TILE_HOPS * N_SUB - 1;
            off = PITCH - 16;
        }
        const unsigned r = N_SUB == 1 ? q : q % WIDE_TILE_HOPS, j = N_SUB == 1 ? 0u : q / WIDE_TILE_HOPS;
        long so = (((hop0 + (long)r) * hop_bytes + mis) & ~15L) + (long)(j * (unsigned)WIN_BYTES) + (long)(seg * S) + (long)off;
        if (so + 16 > span_end) so = span_end - 16;
        if (so < 0) so = 0;
        return so;
    }

    /* Image byte that holds byte k (0 <= k < WIN_BYTES, inside segment `seg`) of window piece `piece` of the tile's hop `row`, for a row with delta = 0; the
     * reader adds the row's delta. */
    static AB_WIDE_HD int frag(int row, int piece, int seg, int k) {
        return SEG == 1 ? row * PITCH + piece * WIN_BYTES + k : (piece * WIDE_TILE_HOPS + row) * PITCH + (k - seg * S);
    }
};

}  // namespace airband
#endif
