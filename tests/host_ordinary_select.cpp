// TEST INFRASTRUCTURE: the rules by which an unflagged handle picks an instantiation of the ordinary matrix-core channelizers (csrc/channelizer_dft.hip,
// csrc/channelizer_f32.hip), as the LIBRARY has them: tests/test_ordinary_variants.py builds this file with g++ into a shared library that is linked against
// libairband_hip.so and calls it through ctypes.  Nothing is restated here: the inline rules come from csrc/kernels.h, the others are the library's own symbols.
#include "kernels.h"

using namespace airband;

extern "C" {

int ordsel_dft_supported(int fft_size, int hop_bytes, int sfmt, int max_ch) { return dft_supported(fft_size, hop_bytes, sfmt, max_ch) ? 1 : 0; }
int ordsel_dft_nbuf(int hop_bytes, int win_bytes, int np) { return dft_nbuf(hop_bytes, win_bytes, np); }
int ordsel_dft_sub(int hop_bytes, int win_bytes, int np) { return dft_sub(hop_bytes, win_bytes, np); }
int ordsel_dft_lds_per_buf(int hop_bytes, int win_bytes, int np) { return dft_lds_per_buf(hop_bytes, win_bytes, np); }
int ordsel_f32_supported(int fft_size, int hop_samples, int sfmt) { return f32_supported(fft_size, hop_samples, sfmt) ? 1 : 0; }
int ordsel_f32_layout(int fft_size, int hop_bytes) { return f32_layout(fft_size, hop_bytes); }
int ordsel_f32_small_tile(int fft_size, int hop_bytes) { return f32_small_tile(fft_size, hop_bytes) ? 1 : 0; }
int ordsel_f32_n_seg(int fft_size) { return f32_n_seg(fft_size); }

}
