// Host build of csrc/kernels/murmur3.h against known answers.  Arguments: triples
// <bytes in hex, "-" for none> <seed in hex> <hash in hex>.  For every triple the byte-loader
// template, the host pointer version and a hand composition of the three steps must all give the
// hash.  Exit status: the number of triples that did not (0 = all good), 255 for bad arguments.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../csrc/kernels/murmur3.h"

static uint32_t by_steps(const uint8_t* p, int len, uint32_t seed) {
    uint32_t h = seed;
    for (int i = 0; i + 4 <= len; i += 4)
        h = hm::mm_chain(h, hm::mm_premix((uint32_t)p[i] | (uint32_t)p[i + 1] << 8 | (uint32_t)p[i + 2] << 16 |
                                          (uint32_t)p[i + 3] << 24));
    h ^= hm::mm_premix(hm::mm_tail_word(p + (len & ~3), len & 3));
    return hm::mm_fmix(h, (uint32_t)len);
}

int main(int argc, char** argv) {
    if (argc < 4 || (argc - 1) % 3) return 255;
    int bad = 0;
    for (int a = 1; a < argc; a += 3) {
        std::vector<uint8_t> bytes;
        const char* hex = argv[a];
        if (strcmp(hex, "-") != 0) {
            if (strlen(hex) % 2) return 255;
            for (size_t i = 0; hex[i]; i += 2) {
                const char b[3] = {hex[i], hex[i + 1], 0};
                bytes.push_back((uint8_t)strtoul(b, nullptr, 16));
            }
        }
        bytes.push_back(0xA5);                       // one byte past the end: never part of the hash
        const uint8_t* p = bytes.data();
        const int len = (int)bytes.size() - 1;
        const uint32_t seed = (uint32_t)strtoul(argv[a + 1], nullptr, 16);
        const uint32_t want = (uint32_t)strtoul(argv[a + 2], nullptr, 16);
        const uint32_t loader = hm::murmur3([p](int i) { return p[i]; }, len, seed);
        const uint32_t pointer = hm::murmur3_bytes(p, len, seed);
        const uint32_t steps = by_steps(p, len, seed);
        if (loader != want || pointer != want || steps != want) {
            printf("MISMATCH %s seed %08x: want %08x, loader %08x, pointer %08x, steps %08x\n", hex, seed, want,
                   loader, pointer, steps);
            ++bad;
        }
    }
    printf("checked %d bad %d\n", (argc - 1) / 3, bad);
    return bad > 254 ? 254 : bad;
}
