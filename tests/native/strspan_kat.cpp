// Host build of the word loaders and mm3 of csrc/kernels/strspan.h.
//   1. Grid: a string at every start position 0..15 of a 64-byte array, every length 0..40 and
//      four seeds; the bytes around it are 0xFF, so a loader that fails to mask the tail is
//      caught.  mm3 over LdsWords (the aligned dword of the first byte and its bit shift) and over
//      GlobalWords must both equal hm::murmur3_bytes.
//   2. Arguments: triples <bytes in hex, "-" for none> <seed in hex> <hash in hex>; mm3 over both
//      loaders must give the hash.
// Exit status: the number of failures (0 = all good), 255 for bad arguments.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../csrc/kernels/strspan.h"

static uint32_t words[16];                            // 64 bytes, dword aligned
static uint8_t* const bytes = reinterpret_cast<uint8_t*>(words);

static void place(int pos, const uint8_t* src, int len) {
    memset(bytes, 0xFF, sizeof(words));
    memcpy(bytes + pos, src, (size_t)len);
}

static uint32_t by_lds(int pos, int len, uint32_t seed) {
    return hm::mm3(hm::LdsWords{words + (pos >> 2), 8 * (pos & 3)}, len, seed);
}

static uint32_t by_global(int pos, int len, uint32_t seed) {
    return hm::mm3(hm::GlobalWords{bytes + pos, len}, len, seed);
}

int main(int argc, char** argv) {
    if ((argc - 1) % 3) return 255;
    int bad = 0, grid = 0;
    const uint32_t seeds[4] = {0u, 1u, 0x9747B28Cu, 0xFFFFFFFFu};
    uint8_t text[44];                                 // pos 15 + 44 bytes + the dword pair's reach < 64
    for (int pos = 0; pos < 16; ++pos)
        for (int len = 0; len <= 40; ++len) {
            for (int i = 0; i < len; ++i) text[i] = (uint8_t)(37 * i + 11 * pos + 5 * len + 1);
            place(pos, text, len);
            for (uint32_t seed : seeds) {
                const uint32_t want = hm::murmur3_bytes(text, len, seed);
                const uint32_t lds = by_lds(pos, len, seed), glb = by_global(pos, len, seed);
                ++grid;
                if (lds != want || glb != want) {
                    printf("MISMATCH pos %d len %d seed %08x: want %08x, lds %08x, global %08x\n", pos, len, seed,
                           want, lds, glb);
                    ++bad;
                }
            }
        }
    for (int a = 1; a < argc; a += 3) {
        const char* hex = argv[a];
        int len = 0;
        if (strcmp(hex, "-") != 0) {
            if (strlen(hex) % 2 || strlen(hex) / 2 > sizeof(text)) return 255;
            for (size_t i = 0; hex[i]; i += 2) {
                const char b[3] = {hex[i], hex[i + 1], 0};
                text[len++] = (uint8_t)strtoul(b, nullptr, 16);
            }
        }
        const uint32_t seed = (uint32_t)strtoul(argv[a + 1], nullptr, 16);
        const uint32_t want = (uint32_t)strtoul(argv[a + 2], nullptr, 16);
        for (int pos = 0; pos < 16; pos += 5) {       // 0, 5, 10, 15: every position in a dword
            place(pos, text, len);
            const uint32_t lds = by_lds(pos, len, seed), glb = by_global(pos, len, seed);
            if (lds != want || glb != want) {
                printf("MISMATCH %s seed %08x pos %d: want %08x, lds %08x, global %08x\n", hex, seed, pos, want,
                       lds, glb);
                ++bad;
            }
        }
    }
    printf("grid %d vectors %d bad %d\n", grid, (argc - 1) / 3, bad);
    return bad > 254 ? 254 : bad;
}
