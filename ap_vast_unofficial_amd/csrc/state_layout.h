// Host-side layouts of the named state arrays, for both streams (stream_state.hip, stream_bb.hip).  Plain C++: nothing here
// knows the device.  All sizes count elements of esz bytes.
#pragma once
#include <cstddef>
#include <cstring>

// A ring buffer of `rows` rows of `len` elements keeps logical element 0 of every row at physical index `off` (0 <= off < len):
// logical [0, len - off) = physical [off, len), logical [len - off, len) = physical [0, off).  Callers get and give logical order.
inline void ring_to_logical(void* dst, const void* src, size_t rows, size_t len, size_t off, size_t esz) {
    char* out = static_cast<char*>(dst);
    const char* in = static_cast<const char*>(src);
    for (size_t r = 0; r < rows; ++r) {
        std::memcpy(out + (r * len) * esz, in + (r * len + off) * esz, (len - off) * esz);
        std::memcpy(out + (r * len + (len - off)) * esz, in + (r * len) * esz, off * esz);
    }
}

inline void ring_from_logical(void* dst, const void* src, size_t rows, size_t len, size_t off, size_t esz) {
    char* out = static_cast<char*>(dst);
    const char* in = static_cast<const char*>(src);
    for (size_t r = 0; r < rows; ++r) {
        std::memcpy(out + (r * len + off) * esz, in + (r * len) * esz, (len - off) * esz);
        std::memcpy(out + (r * len) * esz, in + (r * len + (len - off)) * esz, off * esz);
    }
}

// Spectra kept in groups of g bins, [ceil(K / g)][C][g] (src: the whole groups), to bin-major [K][C]
inline void grouped_to_bin_major(void* dst, const void* src, size_t K, size_t C, size_t g, size_t esz) {
    char* out = static_cast<char*>(dst);
    const char* in = static_cast<const char*>(src);
    for (size_t k = 0; k < K; ++k)
        for (size_t c = 0; c < C; ++c) std::memcpy(out + (k * C + c) * esz, in + ((k / g) * g * C + c * g + k % g) * esz, esz);
}
