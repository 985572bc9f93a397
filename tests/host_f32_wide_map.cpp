// TEST INFRASTRUCTURE: csrc/f32_wide_map.h -- the address map the CF32 wide-hop kernel calls -- compiled for the host (tests/test_wide_hops_f32.py builds this file
// with g++ into a shared library and calls it through ctypes).  f32wm_walk() stages every (segment, tile, row, 16-byte piece) of a batch into a model of the LDS
// image that remembers, per image byte, the stream byte it came from, then performs every fragment read of every wave and lane group, and checks what the kernel
// relies on.  Returns 0, or the number of the first check that failed (`where` then holds its coordinates).
#include <cstdint>
#include <vector>

#include "f32_wide_map.h"

using namespace airband;

extern "C" {

// out[0] = pitch, [1] = image bytes, [2] = LDS total, [3] = waves, [4] = plan segments of fft_size, [5] = row pieces (even hop), [6] = row pieces (odd hop)
int f32wm_geometry(int fft_size, int* out) {
    const int n = f32w_plan_segments(fft_size);
    if (n <= 0) return 1;
    const int S = fft_size / n, NW = f32w_nw(S);
    out[0] = f32w_pitch(S);
    out[1] = f32w_image_bytes(S);
    out[2] = f32w_lds_total(S, NW);
    out[3] = NW;
    out[4] = n;
    out[5] = f32w_row_pieces(S, false);
    out[6] = f32w_row_pieces(S, true);
    return 0;
}

// One batch of n_hops hops whose first ring row is `shift` rows into a 16-row tile; the span starts `mis` bytes behind an aligned 16-byte piece.
// counts[0] = pieces staged, [1] = fragment bytes checked against the stream, [2] = fragment reads checked for bank groups, [3] = 8-byte (half) pieces
int f32wm_walk(int fft_size, long hop_samples, int mis, int n_hops, int shift, long* counts, long* where) {
    const int n_seg = f32w_plan_segments(fft_size);
    if (n_seg <= 0) return 1;
    const int S = fft_size / n_seg, NW = f32w_nw(S), READS = 2 * S / 4 / NW / 4, PIECE = 8 * S / NW;
    const long hop_bytes = 8 * hop_samples;
    const bool odd = (hop_samples & 1) != 0;
    if (!odd && mis != 0) return 2;
    if (odd && mis != 0 && mis != 8) return 2;
    const int image = f32w_image_bytes(S), npr = f32w_row_pieces(S, odd);
    const int tiles = (shift + n_hops + 15) / 16;
    // the bytes of the dongle's span the interface promises, from the span's first byte: the last hop's WHOLE window (batch_bytes + lookahead_bytes is no less)
    const long promised = (long)(n_hops - 1) * hop_bytes + 8L * fft_size;
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    auto fail = [&](int code, long a, long b, long c, long d) {
        where[0] = a; where[1] = b; where[2] = c; where[3] = d;
        return code;
    };
    for (int seg = 0; seg < n_seg; seg++) {
        const long seg_off = (long)seg * 8 * S; // the kernel moves its source pointer on by this much
        const long span_end = f32w_span_end(n_hops, hop_bytes, S, mis);
        for (int t = 0; t < tiles; t++) {
            const long hop0 = (long)t * 16 - shift;
            std::vector<long> img(image, -2); // -2: never written; -1: written, not from the span (the unused half of a half piece)
            for (int row = 0; row < 16; row++)
                for (int col = 0; col < npr; col++) {
                    int nb = 0;
                    const long so = f32w_src(row, col, hop0, hop_bytes, mis, span_end, &nb);
                    if (so < 0 || (so & 15) || (nb != 16 && nb != 8)) return fail(10, seg, t, row, col);
                    if (!odd && nb != 16) return fail(11, seg, t, row, col);
                    // from the span's first byte: at most 15 bytes in front of it, never past what the interface promises
                    const long first = seg_off + so - mis, last = first + nb;
                    if (first < -15 || last > promised) return fail(12, seg, t, row, first);
                    const int p = f32w_park(S, row, col);
                    if (p < 0 || p + 16 > image || (p & 15)) return fail(13, seg, t, row, col);
                    for (int b = 0; b < 16; b++) {
                        if (img[p + b] != -2) return fail(14, seg, t, row, col); // an image byte is staged once
                        img[p + b] = b < nb ? so + b : -1;
                    }
                    counts[0]++;
                    counts[3] += nb == 8;
                }
            // every fragment read of every wave (piece), lane group and step, for the 16 rows = the 16 lanes of a group
            for (int piece = 0; piece < NW; piece++)
                for (int grp = 0; grp < 4; grp++)
                    for (int j = 0; j < READS; j++) {
                        unsigned seen = 0;
                        for (int row = 0; row < 16; row++) {
                            const long hop = hop0 + row;
                            const int delta = odd ? f32w_delta(hop, hop_bytes, mis) : 0;
                            if (delta != f32w_delta((long)row - shift, hop_bytes, mis)) return fail(20, seg, t, row, delta); // the same in every tile: the kernel computes it once
                            const int a = f32w_frag(S, NW, row, delta, piece, grp, j);
                            if (a < 0 || a + 16 > image || (a & (odd ? 7 : 15))) return fail(21, seg, t, row, a);
                            // 64 banks of 4 bytes = 16 groups of 16 bytes: the 16 rows of a read must fall in 16 different ones (odd hops: the group in which
                            // a row's two 8-byte halves start; a row that starts 8 bytes in ends in the next group, which is the next row's neighbour's, not its own)
                            const unsigned bit = 1u << ((unsigned)(a % 256) / 16);
                            if (seen & bit) return fail(23, seg, t, piece, j);
                            seen |= bit;
                            if (hop < 0 || hop >= n_hops) continue; // computed and dropped
                            for (int b = 0; b < 16; b++) {
                                const long k = (long)piece * PIECE + 64 * j + 16 * grp + b; // byte of the staged segment
                                if (img[a + b] != hop * hop_bytes + mis + k) return fail(24, seg, t, row, k);
                                counts[1]++;
                            }
                        }
                        counts[2]++;
                    }
            // (piece, grp, j) -> k = piece PIECE + 64 j + 16 grp + [0, 16) covers [0, 8 S) exactly once: every window byte of a row is read once, and was staged once
            if ((long)NW * 4 * READS * 16 != 8L * S) return fail(30, seg, t, 0, 0);
        }
    }
    return 0;
}

}
