// TEST INFRASTRUCTURE: csrc/dft_wide_map.h -- the address map the wide-hop kernel calls -- compiled for the host (tests/test_wide_windows.py builds this file with
// g++ into a temporary directory).  Nothing is restated here: every function hands the header's own result out.
#include <stdint.h>

#include "dft_wide_map.h"

using namespace airband;

namespace {

// (bytes per window piece, pieces, segments): CS16 fft 2048, u8 / s8 fft 4096, CS16 fft 4096, and CS16 fft 512 as the one-segment control; then every other shape
// launch_channelizer_dft_wide() can select -- u8 / s8 fft 256, u8 / s8 fft 512, CS16 fft 256 (the same map, walked with CS16 hops), u8 / s8 fft 1024, CS16 fft 1024,
// u8 / s8 fft 2048
template <class F>
int with_shape(int shape, F&& f) {
    switch (shape) {
    case 0: return f(WideMap<2048, 4, 2>{});
    case 1: return f(WideMap<1024, 8, 2>{});
    case 2: return f(WideMap<2048, 8, 4>{});
    case 3: return f(WideMap<2048, 1, 1>{});
    case 4: return f(WideMap<512, 1, 1>{});
    case 5: return f(WideMap<1024, 1, 1>{});
    case 6: return f(WideMap<1024, 1, 1>{});
    case 7: return f(WideMap<1024, 2, 1>{});
    case 8: return f(WideMap<2048, 2, 1>{});
    case 9: return f(WideMap<1024, 4, 1>{});
    default: return -1;
    }
}

}  // namespace

extern "C" {

// out[0..6] = N_SUB, S, PITCH, IMAGE, N_DMA, wide_lds_total(), wide_plan_segments()
int wm_geometry(int shape, int win_bytes, int np, int seg, int* out) {
    return with_shape(shape, [&](auto m) {
        typedef decltype(m) M;
        out[0] = M::N_SUB; out[1] = M::S; out[2] = M::PITCH; out[3] = M::IMAGE; out[4] = M::N_DMA;
        out[5] = wide_lds_total(win_bytes, np, seg);
        out[6] = wide_plan_segments(win_bytes, np);
        return 0;
    });
}

long wm_span_end(int n_hops, long hop_bytes, int win_all, int mis) { return wide_span_end(n_hops, hop_bytes, win_all, mis); }

int wm_delta(long hop, long hop_bytes, int mis) { return wide_delta(hop, hop_bytes, mis); }

// out[i * 64 + l] = source offset of transfer i, lane l (image bytes [1024 i + 16 l, + 16)); out holds N_DMA x 64 values
int wm_sources(int shape, long hop0, long hop_bytes, int mis, int seg, long span_end, long* out) {
    return with_shape(shape, [&](auto m) {
        typedef decltype(m) M;
        for (int i = 0; i < M::N_DMA; i++)
            for (int l = 0; l < 64; l++) out[i * 64 + l] = M::src((unsigned)(i * WIDE_DMA_BYTES + l * 16), hop0, hop_bytes, mis, seg, span_end);
        return 0;
    });
}

// out[(row * np + piece) * (S / 16) + c] = image byte of k = seg * S + 16 c of (row, piece), delta = 0
int wm_frags(int shape, int np, int seg, int* out) {
    return with_shape(shape, [&](auto m) {
        typedef decltype(m) M;
        for (int row = 0; row < WIDE_TILE_HOPS; row++)
            for (int piece = 0; piece < np; piece++)
                for (int c = 0; c < M::S / 16; c++) out[(row * np + piece) * (M::S / 16) + c] = M::frag(row, piece, seg, seg * M::S + 16 * c);
        return 0;
    });
}

}
