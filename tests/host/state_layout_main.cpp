// Drives csrc/state_layout.h for tests/test_cpu_state_layout.py: the input array comes on standard input, the result goes to
// standard output, both as raw bytes in heap buffers of exactly the sizes the functions are told (built with the address and
// undefined-behaviour sanitizers, so a byte read or written outside them ends the program).
//   to_logical   rows len off esz     ring_to_logical
//   from_logical rows len off esz     ring_from_logical
//   round_trip   rows len off esz     ring_from_logical(ring_to_logical(x))
//   bin_major    K C g esz            grouped_to_bin_major; the input holds ceil(K / g) whole groups
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "state_layout.h"

int main(int argc, char** argv) {
    if (argc != 6) return 2;
    const std::string what = argv[1];
    const size_t a = std::strtoul(argv[2], nullptr, 10), b = std::strtoul(argv[3], nullptr, 10), c = std::strtoul(argv[4], nullptr, 10),
                 esz = std::strtoul(argv[5], nullptr, 10);
    const bool group = what == "bin_major";
    const size_t n_in = group ? (a + c - 1) / c * c * b * esz : a * b * esz, n_out = a * b * esz;
    std::vector<char> in(n_in), out(n_out);
    if (std::fread(in.data(), 1, n_in, stdin) != n_in || std::fgetc(stdin) != EOF) return 3;
    if (what == "to_logical") ring_to_logical(out.data(), in.data(), a, b, c, esz);
    else if (what == "from_logical") ring_from_logical(out.data(), in.data(), a, b, c, esz);
    else if (what == "round_trip") {
        std::vector<char> mid(n_out);
        ring_to_logical(mid.data(), in.data(), a, b, c, esz);
        ring_from_logical(out.data(), mid.data(), a, b, c, esz);
    } else if (group) grouped_to_bin_major(out.data(), in.data(), a, b, c, esz);
    else return 2;
    return std::fwrite(out.data(), 1, n_out, stdout) == n_out ? 0 : 4;
}
