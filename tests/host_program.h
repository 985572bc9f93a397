// tests/host_program.h -- TEST HARNESS ONLY (included by the stand-alone tests/host_*_harness.cpp programs; never part of, linked into or loaded by the library).
// What those programs share: `<program> <input file> <results file>`, the input read whole and taken apart little-endian, buffers exactly as large as the handle
// would make them, and the check that a guard zone kept its poison.  What differs -- the input's format, the kernel's arguments, the launches and what goes into
// the results file -- stays in each harness.
#ifndef AIRBAND_TESTS_HOST_PROGRAM_H
#define AIRBAND_TESTS_HOST_PROGRAM_H

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace host_program {

struct Reader { // the input file's bytes, taken in order; a file that ends early ends the program with status 2
    const char* program = "";
    std::vector<unsigned char> d;
    size_t at = 0;
    bool done() const { return at >= d.size(); }
    void take(void* out, size_t n) {
        if (at + n > d.size()) {
            std::fprintf(stderr, "%s: the input file ends early\n", program);
            std::exit(2);
        }
        if (n) std::memcpy(out, d.data() + at, n);
        at += n;
    }
    int i32() {
        int v;
        take(&v, 4);
        return v;
    }
};

// usage, the input read into `in`, the results file opened: status 2 where any of it fails
inline void open_io(int argc, char** argv, const char* program, Reader& in, FILE*& out) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s <input> <results>\n", program);
        std::exit(2);
    }
    in.program = program;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) std::exit(2);
    unsigned char buf[1 << 16];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) in.d.insert(in.d.end(), buf, buf + n);
    std::fclose(f);
    out = std::fopen(argv[2], "wb");
    if (!out) std::exit(2);
}

// exactly n elements (a sanitizer sees the first byte behind them, once rounded up to the alignment), 64-byte aligned as hipMalloc's are -- rows and records
// are moved 8 and 16 bytes at a time -- and every byte set to `fill`.  Released with std::free().
template <class T>
T* make(size_t n, int fill) {
    const size_t bytes = ((n ? n : 1) * sizeof(T) + 63) / 64 * 64;
    void* p = std::aligned_alloc(64, bytes);
    if (!p) std::exit(3);
    std::memset(p, fill, bytes);
    return static_cast<T*>(p);
}
template <class T>
T* aligned(size_t n) { return make<T>(n, 0); }

// bytes [from, to) of p still hold `value`: a guard zone, or the poisoned rest of a buffer, came back as it was
inline bool untouched(const void* p, size_t from, size_t to, unsigned char value) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = from; i < to; i++)
        if (b[i] != value) return false;
    return true;
}

}  // namespace host_program

#endif
