// presence_san.cpp -- csrc/presence_rule.h under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU.
//   presence_san word                         every (word count, shift, w): one line `nwords shift w value`
//   presence_san eligible LO HI ROWS SV DV...  one 0 / 1 per group of five
//   presence_san usable TLO THI LO HI...       one 0 / 1 per group of four
// The table's words live in a heap block of exactly their size, so a read before the first or past the last
// word is an error.  Test infrastructure: built and run by tests/test_endpoint_presence_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "presence_rule.h"

// the same three words as WORDS in the test: both end bits of each set, so a funnel that drops or doubles a
// boundary bit shows
static const uint32_t kWords[3] = {0x9E3779B9u | 0x80000001u, 0x7F4A7C15u | 0x80000001u, 0xF39CC060u | 0x80000001u};

int main(int argc, char** argv) {
    if (argc < 2) return fprintf(stderr, "usage: presence_san word | eligible ... | usable ...\n"), 2;
    if (!strcmp(argv[1], "word")) {
        for (int nw = 1; nw <= 3; ++nw) {
            std::vector<uint32_t> t(kWords, kWords + nw);  // exactly nw words
            for (int shift = 0; shift < 64; ++shift)
                for (long long w = -1; w <= nw + 3; ++w)
                    printf("%d %d %lld %u\n", nw, shift, w, capsmi::presence_word(t.data(), nw, shift, w));
        }
        return 0;
    }
    if (!strcmp(argv[1], "eligible")) {
        for (int i = 2; i + 4 < argc; i += 5)
            printf("%d\n", capsmi::presence_eligible(atoi(argv[i + 3]) != 0, atoi(argv[i + 4]) != 0, atoll(argv[i + 2]),
                                                     atoll(argv[i]), atoll(argv[i + 1])) ? 1 : 0);
        return 0;
    }
    if (!strcmp(argv[1], "usable")) {
        for (int i = 2; i + 3 < argc; i += 4)
            printf("%d\n", capsmi::presence_usable(atoll(argv[i]), atoll(argv[i + 1]), atoll(argv[i + 2]),
                                                   atoll(argv[i + 3])) ? 1 : 0);
        return 0;
    }
    return 2;
}
